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
// The action body and the two kernels are templates on Weighted (dq_envb_uf_select_weighted, dq_envb_guided_select_uf_weighted): the same
// volume, still one last open window, decoded by ufw_component<false, true> with the lattice's own (w_space, w_time) -- the launch's pair or the lattice's two
// bytes of a uint8 [n_envs][2] array, clamped to 1 .. UFW_MAX_WEIGHT --, so the last round's time edges to B cost w_time.  The Weighted = false instantiations
// are the unit-weight kernels, instruction for instruction.
// And on Corr (dq_envb_uf_select_correlated, dq_envb_guided_select_uf_correlated): section 25's three passes on that window -- component 0
// dry, component 1 with w_corr on the space edges of that correction, component 0 again with w_corr on the space edges of component 1's -- around
// ufw_component<false, true, true>, one (w_space, w_time, w_corr) per lattice (the launch's, or three bytes of a uint8 [n_envs][3] array).  The two masks are a
// tail of ufw_mask_bytes(depth) bytes behind ufw_layout's, for these two instantiations only; the other four are the kernels of before, instruction for instruction.
#include <type_traits>
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

// The weights of a weighted launch: one pair for all lattices, or a pair per lattice.
struct EnvUfWeights {
    const u8* each;             // != NULL: [2 i] / [2 i + 1] = (w_space, w_time) of lattice i
    int w_space, w_time;
};

// The arguments of a weighted launch are the unweighted ones with the weights behind them; the unweighted kernels take EnvUfArgs itself.
struct EnvUfArgsWeighted : EnvUfArgs {
    EnvUfWeights w;
};

// The weights of a correlated launch: one triple for all lattices, or a triple per lattice.
struct EnvUfWeightsCorr {
    const u8* each;             // != NULL: [3 i] .. [3 i + 2] = (w_space, w_time, w_corr) of lattice i
    int w_space, w_time, w_corr;
};

struct EnvUfArgsCorrelated : EnvUfArgs {
    EnvUfWeightsCorr w;
};
template <bool Weighted, bool Corr = false>
using EnvUfArgsOf = std::conditional_t<Corr, EnvUfArgsCorrelated, std::conditional_t<Weighted, EnvUfArgsWeighted, EnvUfArgs>>;

// The workgroup's own pair, read once and clamped to 1 .. UFW_MAX_WEIGHT: a bad byte of a per-lattice array cannot overrun the growth byte.  Every thread reads
// the same two bytes, so the pair is workgroup-uniform; it lives across the decode in vector registers, as the stream kernels hold theirs.
static __device__ __forceinline__ void env_wide_uf_weights(const EnvUfWeights& w, size_t i, int& w_space, int& w_time) {
    w_space = w.w_space; w_time = w.w_time;
    if (w.each != nullptr) { w_space = w.each[2 * i]; w_time = w.each[2 * i + 1]; }
    w_space = min(max(w_space, 1), UFW_MAX_WEIGHT); w_time = min(max(w_time, 1), UFW_MAX_WEIGHT);
    UFW_IN_VGPR(w_space); UFW_IN_VGPR(w_time);
}

// The workgroup's own triple: the pair clamped as above, w_corr to 1 .. w_space.
static __device__ __forceinline__ void env_wide_uf_weights(const EnvUfWeightsCorr& w, size_t i, int& w_space, int& w_time, int& w_corr) {
    w_space = w.w_space; w_time = w.w_time; w_corr = w.w_corr;
    if (w.each != nullptr) { w_space = w.each[3 * i]; w_time = w.each[3 * i + 1]; w_corr = w.each[3 * i + 2]; }
    w_space = min(max(w_space, 1), UFW_MAX_WEIGHT); w_time = min(max(w_time, 1), UFW_MAX_WEIGHT); w_corr = min(max(w_corr, 1), w_space);
    UFW_IN_VGPR(w_space); UFW_IN_VGPR(w_time); UFW_IN_VGPR(w_corr);
}

// The select body for the lattice whose record is `rec`, by the whole workgroup; returns the action to every thread.  Weighted: the lattice's pair, clamped by
// the caller; the growth's event reduction takes the spare word s_acc[7], since s_acc[6] is this body's own (below).
// Corr: the lattice's triple; the dynamic LDS then holds the two masks behind the layout's bytes, and the two components are decoded in three passes.
template <bool Weighted, bool Corr = false>
static __device__ __forceinline__ int env_wide_uf_action(const EnvUfArgs& p, const u64* __restrict__ rec, u8* smem, int tid, int w_space = 1, int w_time = 1,
                                                         int w_corr = 1) {
    int W = p.W, depth = p.depth, identity = p.identity;
    const int O_META = 3 * W + 1;
    int o_comp = 3 * W + 2;
    if ((rec[O_META] >> 32) & 1) return identity;                   // done: workgroup-uniform, no barrier passed yet
    UfwLayout L = ufw_layout(p.n, p.d2, depth);
    int o_mask = 0;
    if constexpr (Corr) { o_mask = L.bytes; UFW_IN_VGPR(o_mask); }  // the two masks: a tail behind the layout of before
    ufw_layout_in_vgpr(L);
    u32* s_frame = reinterpret_cast<u32*>(smem + L.o_frame);
    u32* s_carry = reinterpret_cast<u32*>(smem + L.o_carry);
    int* s_acc = reinterpret_cast<int*>(smem + L.o_acc);
    u32* s_ring = reinterpret_cast<u32*>(smem + L.o_ring);
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
    UfwGraph G;
    G.n = p.n; G.d2 = p.d2; G.per_round = p.d2 + p.n;
    G.mag_n = ufw_magic(G.n); G.mag_pr = ufw_magic(G.per_round);
    UFW_IN_VGPR(G.n); UFW_IN_VGPR(G.d2); UFW_IN_VGPR(G.per_round); UFW_IN_VGPR(G.mag_n); UFW_IN_VGPR(G.mag_pr);
    const u8 *eu0 = p.c0.eu, *ev0 = p.c0.ev, *eu1 = p.c1.eu, *ev1 = p.c1.ev;
    UFW_IN_VGPR(eu0); UFW_IN_VGPR(ev0); UFW_IN_VGPR(eu1); UFW_IN_VGPR(ev1);
    G.depth = depth; G.B = depth * G.n; G.NN = G.B + 1; G.NE = depth * G.per_round;
    const int n_comp = model == DQ_MODEL_X ? 1 : 2;                 // the X model has no action layer for component 1: its frame is not asked for
    if constexpr (Corr) {
        u32* s_mask = reinterpret_cast<u32*>(smem + o_mask);       // u32 [2][depth][8]: A, B
        int mask_stride = depth * UFW_FRAME_WORDS;
        // X model: component 1 is not decoded, so nobody writes B, and the last pass alone runs under w_corr = w_space, where no bit of B tells: the weighted
        // decode.  Else, without a defect of component 1 in the volume nobody reads A and the dry pass is left out.  Both workgroup-uniform.
        int pass = 2;
        if (model == DQ_MODEL_X) w_corr = w_space;
        else pass = __syncthreads_or(tid < depth * UFW_ROW_WORDS && s_ring[row_stride + tid] != 0) ? 0 : 1;
        UFW_IN_VGPR(mask_stride); UFW_IN_VGPR(pass);
        for (; pass < 3; ++pass) {                                 // components 0, 1, 0
            const int c = pass & 1;
            int dry = pass == 0;
            UFW_IN_VGPR(dry);
            G.eu = c ? eu1 : eu0; G.ev = c ? ev1 : ev0;
            // pass 0 reads B, which nobody has written, under w_corr = w_space: every space edge weighs w_space
            ufw_component<false, true, true>(G, s_ring + c * row_stride, smem, L, tid, depth, true, s_frame + c * UFW_FRAME_WORDS, s_carry + c * UFW_ROW_WORDS,
                                             s_acc + c, s_acc + 4 + c, w_space, w_time, s_acc + 7, pass ? w_corr : w_space, s_mask + (c ? 0 : mask_stride),
                                             s_mask + (c ? mask_stride : 0), dry);
        }
    } else
    for (int c = 0; c < n_comp; ++c) {
        G.eu = c ? eu1 : eu0; G.ev = c ? ev1 : ev0;
        if constexpr (Weighted)
            ufw_component<false, true>(G, s_ring + c * row_stride, smem, L, tid, depth, true, s_frame + c * UFW_FRAME_WORDS, s_carry + c * UFW_ROW_WORDS, s_acc + c,
                                       s_acc + 4 + c, w_space, w_time, s_acc + 7);
        else
            ufw_component(G, s_ring + c * row_stride, smem, L, tid, depth, true, s_frame + c * UFW_FRAME_WORDS, s_carry + c * UFW_ROW_WORDS, s_acc + c, s_acc + 4 + c);
    }
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
__global__ __launch_bounds__(UFW_THREADS) void env_wide_uf_kernel(EnvUfArgsOf<Weighted, Corr> p) {
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    if ((int)blockIdx.x >= p.n_envs) return;                        // workgroup-uniform
    int32_t* out = p.action + i;
    UFW_IN_VGPR(out);
    int a;
    if constexpr (Corr) {
        int w_space, w_time, w_corr;
        env_wide_uf_weights(p.w, i, w_space, w_time, w_corr);
        a = env_wide_uf_action<true, true>(p, p.state + i * p.sw, smem, tid, w_space, w_time, w_corr);
    } else if constexpr (Weighted) {
        int w_space, w_time;
        env_wide_uf_weights(p.w, i, w_space, w_time);
        a = env_wide_uf_action<true>(p, p.state + i * p.sw, smem, tid, w_space, w_time);
    } else a = env_wide_uf_action<false>(p, p.state + i * p.sw, smem, tid);
    if (tid == 0) *out = a;
}

template <bool Weighted = false, bool Corr = false>
__global__ __launch_bounds__(UFW_THREADS) void env_wide_guided_uf_kernel(EnvUfArgsOf<Weighted, Corr> p) {
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    if ((int)blockIdx.x >= p.n_envs) return;                        // workgroup-uniform
    const u64* rec = p.state + i * p.sw;
    u32 w[4];                                                       // the words dq_policy_select_wide draws for the lattice, drawn by every thread
    philox4x32_10((u32)p.t, (u32)(p.t >> 32), p.env_id_base + (u32)blockIdx.x, (u32)DQ_STREAM_POLICY << 16, p.seed0, p.seed1, w);
    const u32 w0 = (u32)__builtin_amdgcn_readfirstlane((int)w[0]), w1 = (u32)__builtin_amdgcn_readfirstlane((int)w[1]);
    const u32 w2 = (u32)__builtin_amdgcn_readfirstlane((int)w[2]);
    const bool explore = p.q == nullptr || (u64)w1 < p.T_eps;
    const bool follow = explore && (u64)w2 < p.T_share;
    int32_t* out = p.action + i;
    u8* flag = p.guided ? p.guided + i : nullptr;
    int a;
    if (follow) {                                                   // workgroup-uniform: the only branch with barriers, the only one that touches LDS
        UFW_IN_VGPR(out); UFW_IN_VGPR(flag);
        if constexpr (Corr) {
            int w_space, w_time, w_corr;
            env_wide_uf_weights(p.w, i, w_space, w_time, w_corr);
            a = env_wide_uf_action<true, true>(p, rec, smem, tid, w_space, w_time, w_corr);
        } else if constexpr (Weighted) {
            int w_space, w_time;
            env_wide_uf_weights(p.w, i, w_space, w_time);
            a = env_wide_uf_action<true>(p, rec, smem, tid, w_space, w_time);
        } else a = env_wide_uf_action<false>(p, rec, smem, tid);
    } else {
        if (tid >= 64) return;                                      // one wave suffices, and no barrier follows
        const u64* lg = rec + 3 * p.W + 2 + p.LW;                   // the record's legal set: what the last reset / step also wrote to its legal_dev
        if (explore) {                                              // policy_wide_kernel's rule
            int n_legal = 0;
            for (int k = 0; k < p.LW; ++k) n_legal += __popcll(lg[k]);
            int kk = (int)__umulhi(w0, (u32)n_legal);
            a = -1;
            for (int k = 0; k < p.LW && a < 0; ++k) {
                u64 m = lg[k];
                const int c = __popcll(m);
                if (kk < c) {
                    for (int s = 0; s < kk; ++s) m &= m - 1;
                    a = 64 * k + __ffsll((long long)m) - 1;
                } else kk -= c;
            }
        } else {                                                    // larger value, the lower index among equals: independent of how many threads share the row
            const float* row = p.q + i * p.n_actions;
            float bv = -INFINITY;
            int ba = EWU_NONE;
            for (int k = tid; k < p.n_actions; k += 64) {
                const bool ok = !p.masked_greedy || ((lg[k >> 6] >> (k & 63)) & 1);
                const float v = row[k];
                if (ok && (v > bv || ba == EWU_NONE)) { bv = v; ba = k; }
            }
            dq_wave_argmax(bv, ba);
            a = __builtin_amdgcn_readfirstlane(ba);
        }
    }
    if (tid == 0) {
        *out = a;
        if (flag) *flag = follow ? 1 : 0;
    }
}

// What both entry points check alike, before any device work: the handles, the decoder's lattice and window (DQ_ERR_INVALID); then the kernels' LDS limit, once per
// device (DQ_ERR_UNSUPPORTED).
dq_status env_wide_uf_prepare(const dq_envb* E, const dq_wide_uf* H, const int32_t* action_dev, const float* q_dev, EnvUfArgs* a, int* lds, const char* who) {
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
        const void* kernels[4] = {reinterpret_cast<const void*>(env_wide_uf_kernel<false>), reinterpret_cast<const void*>(env_wide_guided_uf_kernel<false>),
                                  reinterpret_cast<const void*>(env_wide_uf_kernel<true>), reinterpret_cast<const void*>(env_wide_guided_uf_kernel<true>)};
        // the correlated kernels carry their two masks behind that
        const int lds_max_corr = lds_max + ufw_mask_bytes(EWU_MAX_DEPTH);
        const void* correlated[2] = {reinterpret_cast<const void*>(env_wide_uf_kernel<true, true>),
                                     reinterpret_cast<const void*>(env_wide_guided_uf_kernel<true, true>)};
        hipError_t ea = hipSuccess;
        for (int k = 0; k < 4 && ea == hipSuccess; ++k) ea = hipFuncSetAttribute(kernels[k], hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
        for (int k = 0; k < 2 && ea == hipSuccess; ++k) ea = hipFuncSetAttribute(correlated[k], hipFuncAttributeMaxDynamicSharedMemorySize, lds_max_corr);
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
    *lds = ufw_layout(H->n, H->d2, S.depth).bytes;
    return DQ_OK;
}

// What the weighted forms check on top, before anything else: without a per-lattice array the uniform pair lies in 1 .. UFW_MAX_WEIGHT (an array is the caller's to
// check; the kernel clamps it and does not read the uniform pair).
dq_status env_wide_uf_check_weights(int w_space, int w_time, const uint8_t* weights_each_dev, const char* who) {
    DQ_REQUIRE(weights_each_dev != nullptr || (w_space >= 1 && w_space <= UFW_MAX_WEIGHT && w_time >= 1 && w_time <= UFW_MAX_WEIGHT), DQ_ERR_INVALID,
               "%s: weights (%d, %d) outside 1..%d", who, w_space, w_time, UFW_MAX_WEIGHT);
    return DQ_OK;
}

// ... and the correlated forms: the pair as above, the uniform w_corr in 1 .. w_space.
dq_status env_wide_uf_check_correlated(int w_space, int w_time, int w_corr, const uint8_t* weights_each_dev, const char* who) {
    const dq_status rc = env_wide_uf_check_weights(w_space, w_time, weights_each_dev, who);
    if (rc != DQ_OK) return rc;
    DQ_REQUIRE(weights_each_dev != nullptr || (w_corr >= 1 && w_corr <= w_space), DQ_ERR_INVALID, "%s: w_corr = %d outside 1..w_space = %d", who, w_corr, w_space);
    return DQ_OK;
}

// The select entry points: one body, `who` names the caller in the messages.  ww: the weights of a weighted launch, wc: of a correlated one, both NULL for the
// unit-weight kernel.
dq_status env_wide_uf_select(const char* who, dq_envb* env, dq_wide_uf* H, int32_t* action_dev, void* stream, const EnvUfWeights* ww = nullptr,
                             const EnvUfWeightsCorr* wc = nullptr) {
    EnvUfArgsWeighted a;
    int lds = 0;
    const dq_status rc = env_wide_uf_prepare(env, H, action_dev, nullptr, &a, &lds, who);
    if (rc != DQ_OK) return rc;
    if (wc) {
        EnvUfArgsCorrelated ac;
        static_cast<EnvUfArgs&>(ac) = a; ac.w = *wc;
        env_wide_uf_kernel<true, true><<<a.n_envs, UFW_THREADS, lds + ufw_mask_bytes(a.depth), (hipStream_t)stream>>>(ac);
    } else if (ww) {
        a.w = *ww;
        env_wide_uf_kernel<true><<<a.n_envs, UFW_THREADS, lds, (hipStream_t)stream>>>(a);
    } else env_wide_uf_kernel<false><<<a.n_envs, UFW_THREADS, lds, (hipStream_t)stream>>>(static_cast<const EnvUfArgs&>(a));
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

dq_status env_wide_uf_guided_select(const char* who, dq_envb* env, dq_wide_uf* H, const float* q_dev, double eps, double guide_share, int masked_greedy,
                                    const uint32_t seed[2], uint64_t t, int32_t* action_dev, uint8_t* guided_dev, void* stream, const EnvUfWeights* ww = nullptr,
                                    const EnvUfWeightsCorr* wc = nullptr) {
    DQ_REQUIRE(seed, DQ_ERR_INVALID, "%s: null argument", who);
    DQ_REQUIRE(eps >= 0.0 && eps <= 1.0, DQ_ERR_INVALID, "%s: eps must be in [0,1]", who);                                    // (NaN fails both compares)
    DQ_REQUIRE(guide_share >= 0.0 && guide_share <= 1.0, DQ_ERR_INVALID, "%s: guide_share must be in [0,1]", who);
    EnvUfArgsWeighted a;
    int lds = 0;
    const dq_status rc = env_wide_uf_prepare(env, H, action_dev, q_dev, &a, &lds, who);
    if (rc != DQ_OK) return rc;
    a.q = q_dev; a.T_eps = dq_rate_threshold(eps); a.T_share = dq_rate_threshold(guide_share); a.t = t; a.masked_greedy = masked_greedy;
    a.seed0 = seed[0]; a.seed1 = seed[1]; a.guided = guided_dev;
    if (wc) {
        EnvUfArgsCorrelated ac;
        static_cast<EnvUfArgs&>(ac) = a; ac.w = *wc;
        env_wide_guided_uf_kernel<true, true><<<a.n_envs, UFW_THREADS, lds + ufw_mask_bytes(a.depth), (hipStream_t)stream>>>(ac);
    } else if (ww) {
        a.w = *ww;
        env_wide_guided_uf_kernel<true><<<a.n_envs, UFW_THREADS, lds, (hipStream_t)stream>>>(a);
    } else env_wide_guided_uf_kernel<false><<<a.n_envs, UFW_THREADS, lds, (hipStream_t)stream>>>(static_cast<const EnvUfArgs&>(a));
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

}  // namespace

extern "C" {

dq_status dq_envb_uf_select(dq_envb* env, dq_wide_uf* H, int32_t* action_dev, void* stream) {
    return env_wide_uf_select("dq_envb_uf_select", env, H, action_dev, stream);
}

dq_status dq_envb_uf_select_weighted(dq_envb* env, dq_wide_uf* H, int w_space, int w_time, const uint8_t* weights_each_dev, int32_t* action_dev, void* stream) {
    const dq_status rc = env_wide_uf_check_weights(w_space, w_time, weights_each_dev, "dq_envb_uf_select_weighted");
    if (rc != DQ_OK) return rc;
    const EnvUfWeights ww = {weights_each_dev, w_space, w_time};
    return env_wide_uf_select("dq_envb_uf_select_weighted", env, H, action_dev, stream, &ww);
}

dq_status dq_envb_uf_select_correlated(dq_envb* env, dq_wide_uf* H, int w_space, int w_time, int w_corr, const uint8_t* weights_each_dev, int32_t* action_dev,
                                       void* stream) {
    const dq_status rc = env_wide_uf_check_correlated(w_space, w_time, w_corr, weights_each_dev, "dq_envb_uf_select_correlated");
    if (rc != DQ_OK) return rc;
    const EnvUfWeightsCorr wc = {weights_each_dev, w_space, w_time, w_corr};
    return env_wide_uf_select("dq_envb_uf_select_correlated", env, H, action_dev, stream, nullptr, &wc);
}

dq_status dq_envb_guided_select_uf(dq_envb* env, dq_wide_uf* H, const float* q_dev, double eps, double guide_share, int masked_greedy, const uint32_t seed[2],
                                   uint64_t t, int32_t* action_dev, uint8_t* guided_dev, void* stream) {
    return env_wide_uf_guided_select("dq_envb_guided_select_uf", env, H, q_dev, eps, guide_share, masked_greedy, seed, t, action_dev, guided_dev, stream);
}

dq_status dq_envb_guided_select_uf_weighted(dq_envb* env, dq_wide_uf* H, const float* q_dev, double eps, double guide_share, int masked_greedy,
                                            const uint32_t seed[2], uint64_t t, int w_space, int w_time, const uint8_t* weights_each_dev, int32_t* action_dev,
                                            uint8_t* guided_dev, void* stream) {
    const dq_status rc = env_wide_uf_check_weights(w_space, w_time, weights_each_dev, "dq_envb_guided_select_uf_weighted");
    if (rc != DQ_OK) return rc;
    const EnvUfWeights ww = {weights_each_dev, w_space, w_time};
    return env_wide_uf_guided_select("dq_envb_guided_select_uf_weighted", env, H, q_dev, eps, guide_share, masked_greedy, seed, t, action_dev, guided_dev, stream,
                                     &ww);
}

dq_status dq_envb_guided_select_uf_correlated(dq_envb* env, dq_wide_uf* H, const float* q_dev, double eps, double guide_share, int masked_greedy,
                                              const uint32_t seed[2], uint64_t t, int w_space, int w_time, int w_corr, const uint8_t* weights_each_dev,
                                              int32_t* action_dev, uint8_t* guided_dev, void* stream) {
    const dq_status rc = env_wide_uf_check_correlated(w_space, w_time, w_corr, weights_each_dev, "dq_envb_guided_select_uf_correlated");
    if (rc != DQ_OK) return rc;
    const EnvUfWeightsCorr wc = {weights_each_dev, w_space, w_time, w_corr};
    return env_wide_uf_guided_select("dq_envb_guided_select_uf_correlated", env, H, q_dev, eps, guide_share, masked_greedy, seed, t, action_dev, guided_dev,
                                     stream, nullptr, &wc);
}

}  // extern "C"
