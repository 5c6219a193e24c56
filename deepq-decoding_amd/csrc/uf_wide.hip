// Union-find stream decoding for any odd d in 3 .. 15 with a window of up to 32 rounds (include/deepq_hip.h dq_wide_uf_*): the schedule of
// uf_stream.hip around uf_wide_dev.h's component decode, one workgroup of UFW_THREADS threads per stream.
//   stream_wide_uf_kernel      the rounds are read from memory: thread 128 c + j reads the cell of node j of component c, a wave's ballot is two words of a row
//   stream_run_wide_uf_kernel  the rounds are drawn in the workgroup by tests/decode_eval_ref.sample_volumes' rule (thread q owns qubit q and, for
//                              q < n_stab, stabilizer q's measurement flip): the syndromes never reach memory unless a buffer for them is given
//   verdict_wide_kernel        residual = hidden XOR frame: in code space, homology class, success; no referee is consulted
// The two stream kernels are templates on Closed (dq_wide_uf_decode_closed / dq_wide_uf_run_closed), as uf_stream.hip's are, and on
// (Weighted, Corr), three variants that differ only in what uf_wide.h's ufw_setup and ufw_window do for the flags:
//   <Closed, false, false>  unit weights
//   <Closed, true, false>   DESIGN.md section 23 (dq_wide_uf_*_weighted): an edge of weight w is full at g = 2 w, one (w_space, w_time) per stream
//   <Closed, true, true>    DESIGN.md section 25 (dq_wide_uf_*_correlated): three component decodes per window, 0 dry, 1, 0, each one's space edges cheap
//                           (w_corr) where the one before put its correction; one (w_space, w_time, w_corr) per stream, two masks behind the layout's bytes
// The flags are compile-time: the unit-weight kernels carry no code of the other two.  wide_kernel is the one map from (run, closed, mode) to a kernel.
// The lattice tables come from LatticeHost inside the handle; no environment handle is needed.
#include "uf_wide.h"
#include "lattice_host.h"

#define UFW_MAX_ROUNDS (1 << 20)

namespace {

struct WideArgs {
    UfwComp c0, c1;
    const u8 *node_cell, *node_stab, *cell_stab, *stab_q, *stab_isx;
    int n_streams, d, n, d2, n_stab, G, model, T, window, commit;
    u32 env_id_base, seed0, seed1;
    u64 T_phys, T_meas;
    const u64* T_each;          // != NULL: [2 i] / [2 i + 1] = thresholds of stream i
    const u8* syn_in;           // [n][T][G]                     (stream_wide_uf_kernel)
    u8* syn_out;                // [n][T][G] or NULL             (stream_run_wide_uf_kernel)
    u8* hidden;                 // [n][d2]
    u8* trivial;                // [n]
    u8* frame;                  // [n][d2]
    int32_t *weight, *n_defects, *rounds;      // [n][2] or NULL
};

// The arguments of a weighted or a correlated launch are the unweighted ones with the weights behind them; the unit-weight kernels take WideArgs itself.
struct WideArgsWeighted : WideArgs {
    UfwWeights w;
};
template <bool Weighted>
using WideArgsOf = std::conditional_t<Weighted, WideArgsWeighted, WideArgs>;

// The schedule around a source of rounds: next(j, row0, row1) is called once for every j = 0 .. T - 1, in order, by every thread; it leaves round j's defect
// rows of the two components in the given LDS words (all UFW_ROW_WORDS of each) and may use barriers; `last` says j = T - 1 (the last row of the final window).
// Closed: the stream ends on a round of perfect measurements, so the final window has no time edges in its last round.
// Weighted, Corr: what uf_wide.h's ufw_window decodes per window, with the stream's weights of S; the schedule, the carry and the closed final window are the
// same for all three.
template <bool Closed, bool Weighted, bool Corr, class Next>
static __device__ __forceinline__ void wide_windows(const WideArgs& p, u8* smem, const UfwSetup& S, int tid, Next next) {
    const UfwHead H = ufw_head(smem, S.L);
    u32 *s_frame = H.s_frame, *s_carry = H.s_carry, *s_ring = H.s_ring;
    int* s_acc = H.s_acc;
    int window = p.window, commit = p.commit, T = p.T, row_stride = window * UFW_ROW_WORDS;
    UFW_IN_VGPR(window); UFW_IN_VGPR(commit); UFW_IN_VGPR(T); UFW_IN_VGPR(row_stride);
    if (tid < 2 * UFW_FRAME_WORDS) s_frame[tid] = 0;
    if (tid < 2 * UFW_ROW_WORDS) s_carry[tid] = 0;
    if (tid < 8) s_acc[tid] = 0;
    __syncthreads();
    UfwGraph G = ufw_graph_in_vgpr(p.n, p.d2);
    const UfwEnds E = ufw_ends_in_vgpr(p.c0, p.c1);
    int n_windows = window >= T ? 1 : (T - window + commit - 1) / commit + 1;
    int have = 0, j = 0;                                           // rounds of the window already in the ring; the next round of the stream
    UFW_IN_VGPR(n_windows); UFW_IN_VGPR(have); UFW_IN_VGPR(j);
    for (int k = 0; k < n_windows; ++k) {                          // every bound below is a function of (T, window, commit)
        const int a = k * commit;
        const bool final = a + window >= T;
        const int l = final ? T - a : window;                      // have < l <= window
        for (int t = have; t < l; ++t, ++j) next(j, Closed && final && t == l - 1, s_ring + t * UFW_ROW_WORDS, s_ring + row_stride + t * UFW_ROW_WORDS);
        __syncthreads();
        if (tid < 2 * UFW_ROW_WORDS) {                             // row 0 ^= carry (row 0 leaves the ring with this window: commit >= 1)
            s_ring[(tid >> 2) * row_stride + (tid & 3)] ^= s_carry[tid];
            s_carry[tid] = 0;
        }
        __syncthreads();
        G.depth = l; G.B = l * G.n; G.NN = G.B + 1; G.NE = l * G.per_round;
        ufw_window<Closed, Weighted, Corr>(G, E, smem, S, H, tid, row_stride, commit, final, 2, s_acc + 6);
        if (final) break;
        // the ring moves down by `commit` rows (2 window UFW_ROW_WORDS <= UFW_THREADS words)
        const int keep = window - commit;
        u32 r = 0;
        const int row = (tid >> 2) % window;
        const bool moves = tid < 2 * row_stride && row < keep;
        if (moves) r = s_ring[tid + commit * UFW_ROW_WORDS];
        __syncthreads();
        if (moves) s_ring[tid] = r;
        __syncthreads();
        have = keep;
    }
}

// Where a thread stores its share of a stream's results: computed at the start, so that the base pointers do not live across the decode.
struct WidePtrs {
    u8* frame;                                                     // thread < d2: the thread's cell of frame [n][d2]
    int32_t *weight, *n_defects, *rounds;                          // thread < 2: the thread's entry of [n][2], or NULL
    int has_cell;                                                  // thread < d2
};

static __device__ __forceinline__ WidePtrs wide_ptrs(const WideArgs& p, size_t i, int tid) {
    WidePtrs P;
    const int c = tid & 1;
    P.frame = p.frame + i * p.d2 + (tid < p.d2 ? tid : 0);
    P.weight = p.weight ? p.weight + 2 * i + c : nullptr;
    P.n_defects = p.n_defects ? p.n_defects + 2 * i + c : nullptr;
    P.rounds = p.rounds ? p.rounds + 2 * i + c : nullptr;
    P.has_cell = tid < p.d2;
    UFW_IN_VGPR(P.frame); UFW_IN_VGPR(P.weight); UFW_IN_VGPR(P.n_defects); UFW_IN_VGPR(P.rounds); UFW_IN_VGPR(P.has_cell);
    return P;
}

static __device__ __forceinline__ void wide_store(const WidePtrs& P, u8* smem, const UfwLayout& L, int tid, int nd) {
    const u32* s_frame = reinterpret_cast<const u32*>(smem + L.o_frame);
    int* s_acc = reinterpret_cast<int*>(smem + L.o_acc);
    if ((tid & 63) == 0 && nd) __hip_atomic_fetch_add(s_acc + 2 + (tid >> 7), nd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (P.has_cell) {                                               // hidden_state codes: component 0 = X (1), component 1 = Z (3), both = Y (2)
        const int x = (s_frame[tid >> 5] >> (tid & 31)) & 1, z = (s_frame[UFW_FRAME_WORDS + (tid >> 5)] >> (tid & 31)) & 1;
        *P.frame = (u8)(x ? (z ? 2 : 1) : (z ? 3 : 0));
    }
    if (tid < 2) {
        if (P.weight) *P.weight = s_acc[tid];
        if (P.n_defects) *P.n_defects = s_acc[2 + tid];
        if (P.rounds) *P.rounds = s_acc[4 + tid];
    }
}

template <bool Closed, bool Weighted = false, bool Corr = false>
__global__ __launch_bounds__(UFW_THREADS) void stream_wide_uf_kernel(WideArgsOf<Weighted> p) {
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    if ((int)blockIdx.x >= p.n_streams) return;                     // workgroup-uniform
    const UfwSetup S = ufw_setup<Weighted, Corr>(p, i, p.n, p.d2, p.window);
    const int my_cell = p.node_cell[tid];
    const bool mine = (tid & (UFW_NODE_SLOTS - 1)) < p.n;            // (255 is a cell of the d = 15 grid: the table's padding does not tell)
    const u8* vp = p.syn_in + i * (size_t)p.T * p.G + (mine ? my_cell : 0);
    const WidePtrs P = wide_ptrs(p, i, tid);
    int prev = 0, nd = 0, G = p.G;
    UFW_IN_VGPR(vp); UFW_IN_VGPR(prev); UFW_IN_VGPR(nd); UFW_IN_VGPR(G);
    wide_windows<Closed, Weighted, Corr>(p, smem, S, tid, [&](int j, bool, u32* row0, u32* row1) {
        const int cur = vp[(size_t)j * G] != 0;                    // (a thread without a node reads cell 0 of its own stream and masks it)
        wide_rows(mine ? cur : 0, prev, tid, row0, row1, nd);
    });
    wide_store(P, smem, S.L, tid, nd);
}

template <bool Closed, bool Weighted = false, bool Corr = false>
__global__ __launch_bounds__(UFW_THREADS) void stream_run_wide_uf_kernel(WideArgsOf<Weighted> p) {
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    if ((int)blockIdx.x >= p.n_streams) return;                     // workgroup-uniform
    const UfwSetup S = ufw_setup<Weighted, Corr>(p, i, p.n, p.d2, p.window);
    u8* s_ex = smem + S.L.o_ex;
    u8* s_ez = smem + S.L.o_ez;
    u8* s_v = smem + S.L.o_v;
    u64 T_phys = p.T_phys, T_meas = p.T_meas;
    if (p.T_each != nullptr) { T_phys = p.T_each[2 * i]; T_meas = p.T_each[2 * i + 1]; }
    int has_q = tid < p.d2, has_s = tid < p.n_stab;
    int q4[4] = {255, 255, 255, 255};
    int isx = 0;
    if (has_s) {
#pragma unroll
        for (int k = 0; k < 4; ++k) q4[k] = p.stab_q[4 * tid + k];
        isx = p.stab_isx[tid] != 0;
    }
    const int my_stab = (tid & (UFW_NODE_SLOTS - 1)) < p.n ? p.node_stab[tid] : 255;      // thread 128 c + j: the stabilizer of node j of component c
    const int cs = tid < p.G ? p.cell_stab[tid] : 255;              // thread < G: the stabilizer its cell shows
    u8* syn = p.syn_out && tid < p.G ? p.syn_out + i * (size_t)p.T * p.G + tid : nullptr;
    u32 id = p.env_id_base + (u32)blockIdx.x, seed0 = p.seed0, seed1 = p.seed1;
    int model = p.model, G = p.G;
    UFW_IN_VGPR(T_phys); UFW_IN_VGPR(T_meas); UFW_IN_VGPR(id); UFW_IN_VGPR(seed0); UFW_IN_VGPR(seed1); UFW_IN_VGPR(model); UFW_IN_VGPR(G);
    u8* hid = p.hidden + i * p.d2 + (has_q ? tid : 0);
    u8* triv = p.trivial + i;
    const WidePtrs P = wide_ptrs(p, i, tid);
    int x = 0, z = 0, prev = 0, seen = 0, nd = 0;
    UFW_IN_VGPR(has_q); UFW_IN_VGPR(has_s); UFW_IN_VGPR(isx); UFW_IN_VGPR(x); UFW_IN_VGPR(z); UFW_IN_VGPR(prev); UFW_IN_VGPR(seen); UFW_IN_VGPR(nd);
    UFW_IN_VGPR(hid); UFW_IN_VGPR(triv); UFW_IN_VGPR(syn);
    wide_windows<Closed, Weighted, Corr>(p, smem, S, tid, [&](int j, bool last, u32* row0, u32* row1) {
        u32 w[4];                                                  // sample_volumes' round, round counter j
        philox4x32_10((u32)j, 0u, id, (u32)tid, seed0, seed1, w);
        const bool hit = has_q && (u64)w[0] < T_phys;
        const int typ = model == DQ_MODEL_X ? 1 : 1 + (int)__umulhi(w[1], 3u);
        const bool zhit = has_q && (u64)w[1] < T_phys;
        x ^= (int)(model == DQ_MODEL_IIDXZ ? hit : hit && typ != 3);
        z ^= (int)(model == DQ_MODEL_IIDXZ ? zhit : hit && typ != 1);
        s_ex[tid] = (u8)x; s_ez[tid] = (u8)z;
        __syncthreads();
        if (has_s) {
            const u8* plane = isx ? s_ex : s_ez;
            int par = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) par ^= q4[k] < 255 ? plane[q4[k]] : 0;
            const int v = (par & 1) ^ (int)(!(Closed && last) && (u64)w[2] < T_meas);      // (closed: the last round is read without error, its data errors land)
            seen |= v;
            s_v[tid] = (u8)v;
        }
        __syncthreads();
        if (syn) syn[(size_t)j * G] = cs < 255 ? s_v[cs] : (u8)0;
        const int cur = my_stab < 255 && s_v[my_stab] != 0;
        wide_rows(cur, prev, tid, row0, row1, nd);
    });
    const int any_seen = __syncthreads_or(seen);
    if (has_q) *hid = (u8)(x ? (z ? 2 : 1) : (z ? 3 : 0));
    if (tid == 0) *triv = (u8)(any_seen == 0);
    wide_store(P, smem, S.L, tid, nd);
}

struct WideVerdictArgs {
    const u8 *stab_q, *stab_isx;
    int n_streams, d, d2, n_stab;
    const u8* hidden;           // [n][d2] codes 0..3
    const u8* frame;            // [n][d2] or NULL (no correction)
    u8* verdict;                // [n]
};

__global__ __launch_bounds__(UFW_THREADS) void verdict_wide_kernel(WideVerdictArgs p) {
    __shared__ u8 s_x[UFW_THREADS], s_z[UFW_THREADS];
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    if ((int)blockIdx.x >= p.n_streams) return;                     // workgroup-uniform
    int h = 0, f = 0;
    if (tid < p.d2) {
        h = p.hidden[i * p.d2 + tid] & 3;
        if (p.frame) f = p.frame[i * p.d2 + tid] & 3;
    }
    // codes 1, 2 carry an X component, codes 2, 3 a Z component; the product of two Paulis is the XOR of the components
    const bool x = (h == 1 || h == 2) != (f == 1 || f == 2), z = (h >= 2) != (f >= 2);
    s_x[tid] = (u8)x; s_z[tid] = (u8)z;
    const int row = tid / p.d, col = tid - row * p.d;
    const int cx = __syncthreads_count(x && col == 0) & 1;          // X parity on column 0
    const int cz = __syncthreads_count(z && row == 0) & 1;          // Z parity on row 0
    int par = 0;
    if (tid < p.n_stab) {
        const u8* plane = p.stab_isx[tid] ? s_x : s_z;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int q = p.stab_q[4 * tid + k]; par ^= q < 255 ? plane[q] : 0; }
    }
    const bool in_code = !__syncthreads_or(par & 1);
    const int cls = cx + 2 * cz;
    const bool success = in_code && cls == 0;
    if (tid == 0)                                                   // ALIVE := SUCCESS, decoded field 0: no referee is consulted at these sizes
        p.verdict[i] = (u8)((in_code ? DQ_VERDICT_IN_CODESPACE : 0) | (cls << DQ_VERDICT_CLASS_SHIFT) | (success ? DQ_VERDICT_SUCCESS | DQ_VERDICT_ALIVE : 0));
}

dq_status wide_check(const dq_wide_uf* H, int n, int T, int commit, const int32_t* weight_dev, const int32_t* n_defects_dev, const int32_t* rounds_dev, const char* who) {
    DQ_REQUIRE(n >= 1 && n <= H->max_streams, DQ_ERR_INVALID, "%s: n = %d outside 1..max_streams %d", who, n, H->max_streams);
    DQ_REQUIRE(T >= 1 && T <= UFW_MAX_ROUNDS, DQ_ERR_INVALID, "%s: T = %d outside 1..%d", who, T, UFW_MAX_ROUNDS);
    DQ_REQUIRE(commit >= 1 && commit <= H->window, DQ_ERR_INVALID, "%s: commit = %d outside 1..window %d", who, commit, H->window);
    DQ_REQUIRE(((reinterpret_cast<uintptr_t>(weight_dev) | reinterpret_cast<uintptr_t>(n_defects_dev) | reinterpret_cast<uintptr_t>(rounds_dev)) & 3) == 0,
               DQ_ERR_INVALID, "%s: weight_dev, n_defects_dev and rounds_dev must be 4-byte aligned", who);
    return DQ_OK;
}

void wide_args(const dq_wide_uf* H, int n, int T, int commit, const UfwWeights* w, WideArgsWeighted* a) {
    memset(a, 0, sizeof(*a));
    a->c0 = UfwComp{H->ends, H->ends + 256};
    a->c1 = UfwComp{H->ends + 512, H->ends + 768};
    a->node_cell = H->node_cell; a->node_stab = H->node_stab; a->cell_stab = H->cell_stab; a->stab_q = H->stab_q; a->stab_isx = H->stab_isx;
    a->n_streams = n; a->d = H->d; a->n = H->n; a->d2 = H->d2; a->n_stab = H->n_stab; a->G = H->G; a->model = H->model; a->T = T; a->window = H->window;
    a->commit = commit;
    if (w) a->w = *w;
}

// The one place that maps (run, closed, mode) to a kernel instantiation: f(kernel) gets the __global__ function, whose argument is WideArgs for the unit weights
// and WideArgsWeighted otherwise.  The launches (wide_launch) and dq_wide_uf_create's LDS limits both go through it.
template <class F>
void wide_kernel(bool run, bool closed, UfwMode mode, F&& f) {
    ufw_with_mode(mode, [&](auto weighted, auto corr) {
        constexpr bool W = decltype(weighted)::value, K = decltype(corr)::value;
        if (run) closed ? f(stream_run_wide_uf_kernel<true, W, K>) : f(stream_run_wide_uf_kernel<false, W, K>);
        else closed ? f(stream_wide_uf_kernel<true, W, K>) : f(stream_wide_uf_kernel<false, W, K>);
    });
}

// (a unit-weight kernel takes the WideArgs part of `a`)
void wide_launch(bool run, bool closed, UfwMode mode, const dq_wide_uf* H, const WideArgsWeighted& a, hipStream_t st) {
    const int lds = ufw_lds_bytes(mode, H->lds, H->window);
    wide_kernel(run, closed, mode, [&](auto* kernel) { kernel<<<a.n_streams, UFW_THREADS, lds, st>>>(a); });
}

// The open and the closed entry points: one body, `who` names the caller in the messages.  w: the weights of a weighted or a correlated launch (already
// checked), NULL for the unit-weight kernels.
dq_status wide_decode(bool closed, const char* who, dq_wide_uf* H, const uint8_t* syndromes_dev, int n, int T, int commit, uint8_t* frame_dev, int32_t* weight_dev,
                      int32_t* n_defects_dev, int32_t* rounds_dev, void* stream, UfwMode mode = UFW_UNIT, const UfwWeights* w = nullptr) {
    DQ_REQUIRE(H && syndromes_dev && frame_dev, DQ_ERR_INVALID, "%s: null argument", who);
    const dq_status rc = wide_check(H, n, T, commit, weight_dev, n_defects_dev, rounds_dev, who);
    if (rc != DQ_OK) return rc;
    WideArgsWeighted a;
    wide_args(H, n, T, commit, w, &a);
    a.syn_in = syndromes_dev; a.frame = frame_dev; a.weight = weight_dev; a.n_defects = n_defects_dev; a.rounds = rounds_dev;
    wide_launch(false, closed, mode, H, a, (hipStream_t)stream);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

dq_status wide_run(bool closed, const char* who, dq_wide_uf* H, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys, double p_meas,
                   const double* p_phys_each, const double* p_meas_each, uint8_t* hidden_dev, uint8_t* trivial_dev, uint8_t* frame_dev, int32_t* weight_dev,
                   int32_t* n_defects_dev, int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream, UfwMode mode = UFW_UNIT, const UfwWeights* w = nullptr) {
    DQ_REQUIRE(H && seed && hidden_dev && trivial_dev && frame_dev, DQ_ERR_INVALID, "%s: null argument", who);
    dq_status rc = wide_check(H, n, T, commit, weight_dev, n_defects_dev, rounds_dev, who);
    if (rc != DQ_OK) return rc;
    DQ_REQUIRE((p_phys_each != nullptr) == (p_meas_each != nullptr), DQ_ERR_INVALID, "%s: per-stream rates come as a pair of arrays", who);
    hipStream_t st = (hipStream_t)stream;
    WideArgsWeighted a;
    wide_args(H, n, T, commit, w, &a);
    if (p_phys_each) {
        rc = dq_rate_table_upload(H->rates, n, p_phys_each, p_meas_each, st);
        if (rc != DQ_OK) return rc;
        a.T_each = H->rates.dev;
    } else {
        DQ_REQUIRE(p_phys >= 0.0 && p_phys <= 1.0 && p_meas >= 0.0 && p_meas <= 1.0, DQ_ERR_INVALID, "%s: rates must be in [0,1]", who);
        a.T_phys = dq_rate_threshold(p_phys); a.T_meas = dq_rate_threshold(p_meas);
    }
    a.env_id_base = env_id_base; a.seed0 = seed[0]; a.seed1 = seed[1];
    a.hidden = hidden_dev; a.trivial = trivial_dev; a.frame = frame_dev; a.weight = weight_dev; a.n_defects = n_defects_dev; a.rounds = rounds_dev;
    a.syn_out = syndromes_dev;
    wide_launch(true, closed, mode, H, a, st);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

}  // namespace

extern "C" {

dq_status dq_wide_uf_create(int d, int error_model, int window, int max_streams, dq_wide_uf** out) {
    DQ_REQUIRE(out, DQ_ERR_INVALID, "dq_wide_uf_create: null argument");
    *out = nullptr;
    DQ_REQUIRE(d >= 3 && d <= UFW_MAX_D && (d & 1), DQ_ERR_INVALID, "dq_wide_uf_create: d = %d: odd d in 3..%d", d, UFW_MAX_D);
    DQ_REQUIRE(error_model >= DQ_MODEL_X && error_model <= DQ_MODEL_IIDXZ, DQ_ERR_INVALID, "dq_wide_uf_create: bad error model %d", error_model);
    DQ_REQUIRE(window >= 1 && window <= UFW_MAX_WINDOW, DQ_ERR_INVALID, "dq_wide_uf_create: window = %d outside 1..%d", window, UFW_MAX_WINDOW);
    DQ_REQUIRE(max_streams >= 1, DQ_ERR_INVALID, "dq_wide_uf_create: max_streams must be >= 1");
    LatticeHost Lh;
    lattice_build(d, &Lh);
    const int d2 = d * d, ns = Lh.n_stab, G = (d + 1) * (d + 1), n = (d2 - 1) / 2;
    DQ_REQUIRE((int)Lh.typed[0].size() == n && (int)Lh.typed[1].size() == n && n <= UFW_NODE_SLOTS && G <= UFW_THREADS, DQ_ERR_UNSUPPORTED,
               "dq_wide_uf_create: d = %d: the lattice does not fit a workgroup of %d threads", d, UFW_THREADS);
    const size_t o_ends = 0, o_cell = 1024, o_nstab = o_cell + 256, o_cstab = o_nstab + 256, o_sq = o_cstab + 256, o_isx = o_sq + 1024, bytes = o_isx + 256;
    std::vector<u8> host(bytes, 255), ends;
    lattice_uf_ends(Lh, &ends);
    memcpy(host.data() + o_ends, ends.data(), ends.size());
    for (int c = 0; c < 2; ++c)
        for (int j = 0; j < n; ++j) {
            const int s = Lh.typed[c][j];
            host[o_cell + UFW_NODE_SLOTS * c + j] = (u8)(Lh.sa[s] * (d + 1) + Lh.sb[s]);
            host[o_nstab + UFW_NODE_SLOTS * c + j] = (u8)s;
        }
    for (int cidx = 0; cidx < G; ++cidx) if (Lh.index[cidx] >= 0) host[o_cstab + cidx] = (u8)Lh.index[cidx];
    for (int s = 0; s < ns; ++s) {
        DQ_REQUIRE(Lh.stab_qubits[s].size() <= 4, DQ_ERR_UNSUPPORTED, "dq_wide_uf_create: a stabilizer of more than four qubits");
        for (size_t k = 0; k < Lh.stab_qubits[s].size(); ++k) host[o_sq + 4 * s + k] = (u8)Lh.stab_qubits[s][k];
        host[o_isx + s] = (u8)(Lh.stab_type[s] == 3);
    }
    const UfwLayout L = ufw_layout(n, d2, window);
    // the kernels' limit is the largest shape's, set once per device (common.h dq_device_bit): a handle never lowers what another one launches with
    static unsigned long long attr_devs = 0;
    const unsigned long long dev_bit = dq_device_bit();
    if (!(attr_devs & dev_bit)) {
        const int lds_max = ufw_layout((UFW_MAX_D * UFW_MAX_D - 1) / 2, UFW_MAX_D * UFW_MAX_D, UFW_MAX_WINDOW).bytes;
        const int lds_max_corr = ufw_lds_bytes(UFW_CORRELATED, lds_max, UFW_MAX_WINDOW);      // the correlated kernels carry their two masks behind that
        hipError_t ea = hipSuccess;
        for (int k = 0; k < 12; ++k) {                               // every (run, closed, mode)
            const UfwMode mode = (UfwMode)(k >> 2);
            wide_kernel(k & 1, k & 2, mode, [&](auto* kernel) {
                if (ea == hipSuccess)
                    ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             ufw_lds_bytes(mode, lds_max, UFW_MAX_WINDOW));
            });
        }
        if (ea != hipSuccess) {
            (void)hipGetLastError();
            dq_set_error("dq_wide_uf_create: the device refuses %d bytes of LDS per workgroup: %s", lds_max_corr, hipGetErrorString(ea));
            return DQ_ERR_UNSUPPORTED;
        }
        attr_devs |= dev_bit;
    }
    dq_wide_uf* H = new dq_wide_uf();
    memset(H, 0, sizeof(*H));
    H->d = d; H->model = error_model; H->window = window; H->max_streams = max_streams; H->n = n; H->d2 = d2; H->n_stab = ns; H->G = G; H->lds = L.bytes;
    // the per-stream rate table holds max_streams pairs from the start, as dq_decode_eval_create's does: dq_rate_table_upload never grows it
    const size_t rate_bytes = (2 * (size_t)max_streams + 2) * sizeof(u64);
    hipError_t e = hipMalloc(&H->blob, bytes);
    if (e == hipSuccess) e = hipMemcpy(H->blob, host.data(), bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&H->rates.dev, rate_bytes);
    if (e == hipSuccess) e = hipHostMalloc(&H->rates.host, rate_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&H->rates.copied, hipEventDisableTiming);
    if (e != hipSuccess) {
        dq_set_error("dq_wide_uf_create: table allocation / upload: %s", hipGetErrorString(e));
        dq_wide_uf_destroy(H);
        return e == hipErrorOutOfMemory ? DQ_ERR_NOMEM : DQ_ERR_HIP;
    }
    H->ends = H->blob + o_ends; H->node_cell = H->blob + o_cell; H->node_stab = H->blob + o_nstab; H->cell_stab = H->blob + o_cstab;
    H->stab_q = H->blob + o_sq; H->stab_isx = H->blob + o_isx;
    *out = H;
    return DQ_OK;
}

void dq_wide_uf_destroy(dq_wide_uf* H) {
    if (!H) return;
    dq_rate_table_free(H->rates);
    if (H->blob) (void)hipFree(H->blob);
    delete H;
}

dq_status dq_wide_uf_decode(dq_wide_uf* H, const uint8_t* syndromes_dev, int n, int T, int commit, uint8_t* frame_dev, int32_t* weight_dev, int32_t* n_defects_dev,
                            int32_t* rounds_dev, void* stream) {
    return wide_decode(false, "dq_wide_uf_decode", H, syndromes_dev, n, T, commit, frame_dev, weight_dev, n_defects_dev, rounds_dev, stream);
}

dq_status dq_wide_uf_decode_closed(dq_wide_uf* H, const uint8_t* syndromes_dev, int n, int T, int commit, uint8_t* frame_dev, int32_t* weight_dev,
                                   int32_t* n_defects_dev, int32_t* rounds_dev, void* stream) {
    return wide_decode(true, "dq_wide_uf_decode_closed", H, syndromes_dev, n, T, commit, frame_dev, weight_dev, n_defects_dev, rounds_dev, stream);
}

dq_status dq_wide_uf_run(dq_wide_uf* H, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys, double p_meas,
                         const double* p_phys_each, const double* p_meas_each, uint8_t* hidden_dev, uint8_t* trivial_dev, uint8_t* frame_dev, int32_t* weight_dev,
                         int32_t* n_defects_dev, int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream) {
    return wide_run(false, "dq_wide_uf_run", H, n, T, commit, env_id_base, seed, p_phys, p_meas, p_phys_each, p_meas_each, hidden_dev, trivial_dev, frame_dev, weight_dev,
                    n_defects_dev, rounds_dev, syndromes_dev, stream);
}

dq_status dq_wide_uf_run_closed(dq_wide_uf* H, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys, double p_meas,
                                const double* p_phys_each, const double* p_meas_each, uint8_t* hidden_dev, uint8_t* trivial_dev, uint8_t* frame_dev,
                                int32_t* weight_dev, int32_t* n_defects_dev, int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream) {
    return wide_run(true, "dq_wide_uf_run_closed", H, n, T, commit, env_id_base, seed, p_phys, p_meas, p_phys_each, p_meas_each, hidden_dev, trivial_dev, frame_dev,
                    weight_dev, n_defects_dev, rounds_dev, syndromes_dev, stream);
}

dq_status dq_wide_uf_decode_weighted(dq_wide_uf* H, const uint8_t* syndromes_dev, int n, int T, int commit, int closed, int w_space, int w_time,
                                     const uint8_t* weights_each_dev, uint8_t* frame_dev, int32_t* weight_dev, int32_t* n_defects_dev, int32_t* rounds_dev,
                                     void* stream) {
    const UfwWeights w = {weights_each_dev, w_space, w_time, 1};
    const dq_status rc = ufw_check_weights(UFW_WEIGHTED, closed, w, false, "dq_wide_uf_decode_weighted");
    if (rc != DQ_OK) return rc;
    return wide_decode(closed != 0, "dq_wide_uf_decode_weighted", H, syndromes_dev, n, T, commit, frame_dev, weight_dev, n_defects_dev, rounds_dev, stream,
                       UFW_WEIGHTED, &w);
}

dq_status dq_wide_uf_run_weighted(dq_wide_uf* H, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys, double p_meas,
                                  const double* p_phys_each, const double* p_meas_each, int closed, int w_space, int w_time, const uint8_t* weights_each_dev,
                                  uint8_t* hidden_dev, uint8_t* trivial_dev, uint8_t* frame_dev, int32_t* weight_dev, int32_t* n_defects_dev,
                                  int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream) {
    const UfwWeights w = {weights_each_dev, w_space, w_time, 1};
    const dq_status rc = ufw_check_weights(UFW_WEIGHTED, closed, w, false, "dq_wide_uf_run_weighted");
    if (rc != DQ_OK) return rc;
    return wide_run(closed != 0, "dq_wide_uf_run_weighted", H, n, T, commit, env_id_base, seed, p_phys, p_meas, p_phys_each, p_meas_each, hidden_dev, trivial_dev,
                    frame_dev, weight_dev, n_defects_dev, rounds_dev, syndromes_dev, stream, UFW_WEIGHTED, &w);
}

dq_status dq_wide_uf_decode_correlated(dq_wide_uf* H, const uint8_t* syndromes_dev, int n, int T, int commit, int closed, int w_space, int w_time, int w_corr,
                                       const uint8_t* weights_each_dev, uint8_t* frame_dev, int32_t* weight_dev, int32_t* n_defects_dev, int32_t* rounds_dev,
                                       void* stream) {
    const UfwWeights w = {weights_each_dev, w_space, w_time, w_corr};
    const dq_status rc = ufw_check_weights(UFW_CORRELATED, closed, w, false, "dq_wide_uf_decode_correlated");
    if (rc != DQ_OK) return rc;
    return wide_decode(closed != 0, "dq_wide_uf_decode_correlated", H, syndromes_dev, n, T, commit, frame_dev, weight_dev, n_defects_dev, rounds_dev, stream,
                       UFW_CORRELATED, &w);
}

dq_status dq_wide_uf_run_correlated(dq_wide_uf* H, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys, double p_meas,
                                    const double* p_phys_each, const double* p_meas_each, int closed, int w_space, int w_time, int w_corr,
                                    const uint8_t* weights_each_dev, uint8_t* hidden_dev, uint8_t* trivial_dev, uint8_t* frame_dev, int32_t* weight_dev,
                                    int32_t* n_defects_dev, int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream) {
    const UfwWeights w = {weights_each_dev, w_space, w_time, w_corr};
    const dq_status rc = ufw_check_weights(UFW_CORRELATED, closed, w, false, "dq_wide_uf_run_correlated");
    if (rc != DQ_OK) return rc;
    return wide_run(closed != 0, "dq_wide_uf_run_correlated", H, n, T, commit, env_id_base, seed, p_phys, p_meas, p_phys_each, p_meas_each, hidden_dev, trivial_dev,
                    frame_dev, weight_dev, n_defects_dev, rounds_dev, syndromes_dev, stream, UFW_CORRELATED, &w);
}

dq_status dq_wide_uf_verdict(dq_wide_uf* H, const uint8_t* hidden_dev, const uint8_t* frame_dev, int n, uint8_t* verdict_dev, void* stream) {
    DQ_REQUIRE(H && hidden_dev && verdict_dev, DQ_ERR_INVALID, "dq_wide_uf_verdict: null argument");
    DQ_REQUIRE(n >= 1 && n <= H->max_streams, DQ_ERR_INVALID, "dq_wide_uf_verdict: n = %d outside 1..max_streams %d", n, H->max_streams);
    WideVerdictArgs a;
    memset(&a, 0, sizeof(a));
    a.stab_q = H->stab_q; a.stab_isx = H->stab_isx; a.n_streams = n; a.d = H->d; a.d2 = H->d2; a.n_stab = H->n_stab;
    a.hidden = hidden_dev; a.frame = frame_dev; a.verdict = verdict_dev;
    verdict_wide_kernel<<<n, UFW_THREADS, 0, (hipStream_t)stream>>>(a);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

}  // extern "C"
