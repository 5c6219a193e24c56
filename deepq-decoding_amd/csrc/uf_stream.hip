// Sliding-window union-find decoding of syndrome streams of any length (include/deepq_hip.h dq_stream_decode_uf / dq_stream_run_uf).
// A stream is T rounds of faulty syndromes of one lattice; its defects are D_t = S_t xor S_{t-1} (S_-1 = 0).  With the window w = the handle's volume_depth and
// the commit c: window k starts at round a = k c, is final iff a + w >= T and has l = T - a rounds when final, else w.  Its defect rows are D_a xor carry,
// D_{a+1} .. D_{a+l-1}; uf_dev.h's uf_component_commit decodes it on the depth-l graph, commits the correction's edges of rounds t < c (all of them when
// final) into the frame and the weight, and returns the next carry: the nodes whose time edge of round c - 1 is in the correction.
//   stream_uf_kernel      the rounds are read from memory with uf_st_kernel's ballot front end
//   stream_run_uf_kernel  the rounds are drawn in the wave by eval_sample_kernel's round (decode_eval.hip): stream i is the first T rounds of lattice
//                         env_id_base + i, and the syndromes never reach memory unless a buffer for them is given
// Both kernels are templates on Closed (dq_stream_decode_uf_closed / dq_stream_run_uf_closed): the stream ends on a round of perfect
// measurements -- the final window has no time edges in its last round, and the sampler leaves round T - 1's measurement flips out.
// One wavefront per stream, one wave per block.  The ring of at most 16 defect words per component lives in UF_O_DW of the wave's UF_LDS bytes; the frame
// words, weights, defect counts and growth rounds accumulate in registers.  No scratch, no lock, no loop whose exit depends on another wave: every loop bound
// follows from (T, d, w, c), which the entry points validate.
#include "uf_dev.h"
#include "match_st_dev.h"
#include "decode_eval.h"
#include "env_dev.h"

#define STREAM_MAX_ROUNDS (1 << 20)
// A wave-uniform value that lives across the component decode is kept in a vector register: the decode needs the scalar ones, and a wave of UF_LDS bytes has
// vector registers to spare.
#define STREAM_IN_VGPR(x) asm volatile("" : "+v"(x))

namespace {

// The schedule around a source of rounds: next(j) returns round j's defect ballot D_j (lanes 0 .. n - 1 component 0's nodes, lanes 32 .. component 1's) and is
// called once for every j = 0 .. T - 1, in order; `last` says j = T - 1 (the schedule knows it without T: the last row of the final window).
// Closed: the stream ends on a round of perfect measurements, so the final window has no time edges in its last round.
struct StreamOut {
    u64 m[2];
    int w[2], nd[2], rd[2];
};

template <bool Closed, class Next>
static __device__ __forceinline__ void stream_windows(const UfComp& c0, const UfComp& c1, int T, int window, int commit, u8* smem, int lane, Next next, StreamOut& o) {
    volatile u32* s_dw = reinterpret_cast<volatile u32*>(smem + UF_O_DW);
    o.m[0] = o.m[1] = 0;
    o.w[0] = o.w[1] = o.nd[0] = o.nd[1] = o.rd[0] = o.rd[1] = 0;
    u32 carry0 = 0, carry1 = 0;
    STREAM_IN_VGPR(o.m[0]); STREAM_IN_VGPR(o.m[1]); STREAM_IN_VGPR(o.w[0]); STREAM_IN_VGPR(o.w[1]); STREAM_IN_VGPR(o.nd[0]); STREAM_IN_VGPR(o.nd[1]);
    STREAM_IN_VGPR(o.rd[0]); STREAM_IN_VGPR(o.rd[1]); STREAM_IN_VGPR(carry0); STREAM_IN_VGPR(carry1);
    const int n_windows = window >= T ? 1 : (T - window + commit - 1) / commit + 1;
    int have = 0, j = 0;                                           // rounds of the window already in the ring; the next round of the stream
    STREAM_IN_VGPR(j);
    for (int k = 0; k < n_windows; ++k) {                          // wave-uniform
        const int a = k * commit;
        const bool final = a + window >= T;
        const int l = final ? T - a : window;                      // have < l <= window
        for (int t = have; t < l; ++t, ++j) {
            const u64 D = next(j, Closed && final && t == l - 1);
            o.nd[0] += __popc((u32)D);
            o.nd[1] += __popc((u32)(D >> 32));
            if (lane == 0) { s_dw[t] = (u32)D; s_dw[UF_MAX_DEPTH + t] = (u32)(D >> 32); }
        }
        match_wave_sync();
        if (lane == 0) { s_dw[0] ^= carry0; s_dw[UF_MAX_DEPTH] ^= carry1; }      // (row 0 leaves the ring with this window: commit >= 1)
        match_wave_sync();
#pragma nounroll
        for (int c = 0; c < 2; ++c) {                              // (one copy of the component decode; every branch on c is wave-uniform)
            int w, nd, rd;
            u64 m;
            u32 carry;
            uf_component_commit<Closed>(c ? c1 : c0, l, s_dw + c * UF_MAX_DEPTH, smem, lane, commit, final, w, m, carry, nd, rd);
            if (c) { o.w[1] += w; o.m[1] ^= m; o.rd[1] += rd; carry1 = carry; }
            else { o.w[0] += w; o.m[0] ^= m; o.rd[0] += rd; carry0 = carry; }
        }
        if (final) break;
        // the ring moves down by `commit` rows
        const int keep = window - commit;                          // < 16
        u32 r0 = 0, r1 = 0;
        if (lane < keep) { r0 = s_dw[lane + commit]; r1 = s_dw[UF_MAX_DEPTH + lane + commit]; }
        match_wave_sync();
        if (lane < keep) { s_dw[lane] = r0; s_dw[UF_MAX_DEPTH + lane] = r1; }
        match_wave_sync();
        have = keep;
    }
}

// Where a lane stores its share of a stream's results: computed at the start, so that the base pointers do not live across the decode.
struct StreamPtrs {
    u8* frame;                                                     // lane < d2: the lane's cell of frame [n][d2]
    int32_t *weight, *n_defects, *rounds;                          // lane < 2: the lane's entry of [n][2], or NULL
    int has_cell;                                                  // lane < d2
};

static __device__ __forceinline__ StreamPtrs stream_ptrs(size_t i, int d2, int lane, u8* frame, int32_t* weight, int32_t* n_defects, int32_t* rounds) {
    StreamPtrs P;
    const int c = lane & 1;
    P.frame = frame + i * d2 + (lane < d2 ? lane : 0);
    P.weight = weight ? weight + 2 * i + c : nullptr;
    P.n_defects = n_defects ? n_defects + 2 * i + c : nullptr;
    P.rounds = rounds ? rounds + 2 * i + c : nullptr;
    P.has_cell = lane < d2;
    STREAM_IN_VGPR(P.frame); STREAM_IN_VGPR(P.weight); STREAM_IN_VGPR(P.n_defects); STREAM_IN_VGPR(P.rounds); STREAM_IN_VGPR(P.has_cell);
    return P;
}

static __device__ __forceinline__ void stream_store(const StreamOut& o, const StreamPtrs& P, int lane) {
    if (P.has_cell) {                                               // hidden_state codes: component 0 = X (1), component 1 = Z (3), both = Y (2)
        const int x = (int)((o.m[0] >> lane) & 1), z = (int)((o.m[1] >> lane) & 1);
        *P.frame = (u8)(x ? (z ? 2 : 1) : (z ? 3 : 0));
    }
    if (lane < 2) {
        if (P.weight) *P.weight = lane ? o.w[1] : o.w[0];
        if (P.n_defects) *P.n_defects = lane ? o.nd[1] : o.nd[0];
        if (P.rounds) *P.rounds = lane ? o.rd[1] : o.rd[0];
    }
}

template <bool Closed>
__global__ __launch_bounds__(64) void stream_uf_kernel(UfComp c0, UfComp c1, const u8* __restrict__ cell, const u8* __restrict__ syndromes, int n, int d, int T, int window,
                                                       int commit, u8* __restrict__ frame, int32_t* __restrict__ weight, int32_t* __restrict__ n_defects,
                                                       int32_t* __restrict__ rounds) {
    __shared__ __attribute__((aligned(16))) u8 smem[UF_LDS];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const int G = (d + 1) * (d + 1);
    // lanes 0 .. n - 1 read component 0's nodes, lanes 32 .. 32 + n - 1 component 1's: a ballot is the round's two syndrome words
    const int my_cell = cell[lane];
    const bool mine = my_cell < G;
    const u8* vp = syndromes + (size_t)i * T * G + (mine ? my_cell : 0);
    const StreamPtrs P = stream_ptrs((size_t)i, d * d, lane, frame, weight, n_defects, rounds);
    u64 prev = 0;
    STREAM_IN_VGPR(prev);
    StreamOut o;
    stream_windows<Closed>(c0, c1, T, window, commit, smem, lane, [&](int j, bool) -> u64 {
        const u64 cur = __ballot(mine && vp[(size_t)j * G] != 0);
        const u64 D = cur ^ prev;
        prev = cur;
        return D;
    }, o);
    stream_store(o, P, lane);
}

struct StreamRunArgs {
    const EnvTables* tab;
    UfComp c0, c1;
    const u8* stab;             // MatchStTables::stab: lane 32 c + j -> bit of node j of component c in a syndrome word
    int n, d, d2, n_stab, G, model, T, window, commit;
    u32 env_id_base, seed0, seed1;
    u64 T_phys, T_meas;
    const u64* T_each;          // != NULL: [2 i] / [2 i + 1] = thresholds of stream i
    u8* hidden;                 // [n][d2]
    u8* trivial;                // [n]
    u8* frame;                  // [n][d2]
    int32_t *weight, *n_defects, *rounds;      // [n][2] or NULL
    u8* syndromes;              // [n][T][G] or NULL
};

template <bool Closed>
__global__ __launch_bounds__(64) void stream_run_uf_kernel(StreamRunArgs p) {
    __shared__ __attribute__((aligned(16))) u8 smem[UF_LDS];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= p.n) return;
    const EnvTables* __restrict__ E = p.tab;
    const u64 sq = E->stab_qmask[lane];
    const bool isx = E->stab_isx[lane] != 0;
    int sidx = 255;                                                // eval_sample_kernel's cell -> stabilizer map, for the optional syndromes
    if (lane < p.G) {
        const int a = lane / (p.d + 1), b = lane - a * (p.d + 1);
        sidx = E->cell_stab[2 * a * (2 * p.d + 1) + 2 * b];
    }
    const int my_bit = p.stab[lane];
    u64 T_phys = p.T_phys, T_meas = p.T_meas;
    if (p.T_each != nullptr) { T_phys = p.T_each[2 * (size_t)i]; T_meas = p.T_each[2 * (size_t)i + 1]; }
    u64 xmask = 0, zmask = 0, summed = 0, prev = 0;
    // per-lane forms of the round's lane predicates (a predicate kept across the decode costs a scalar register pair): a lane without a qubit / a stabilizer
    // has the threshold 0, a lane without a node picks no bit, a lane reads the plane its stabilizer measures through a mask
    u64 Tq = lane < p.d2 ? T_phys : 0ull, Tm = lane < p.n_stab ? T_meas : 0ull, selx = isx ? ~0ull : 0ull;
    u32 node_ok = my_bit < 64 ? 1u : 0u, cell_ok = sidx < 64 ? 1u : 0u;
    int model = p.model;
    STREAM_IN_VGPR(Tq); STREAM_IN_VGPR(Tm); STREAM_IN_VGPR(selx); STREAM_IN_VGPR(node_ok); STREAM_IN_VGPR(cell_ok); STREAM_IN_VGPR(model);
    STREAM_IN_VGPR(xmask); STREAM_IN_VGPR(zmask); STREAM_IN_VGPR(summed); STREAM_IN_VGPR(prev);
    u32 seed0 = p.seed0, seed1 = p.seed1, id = p.env_id_base + (u32)i;                          // (the ten rounds' keys are loop invariants: twenty registers)
    STREAM_IN_VGPR(seed0); STREAM_IN_VGPR(seed1); STREAM_IN_VGPR(id);
    const int G = p.G, d2 = p.d2;
    u8* syn = p.syndromes && lane < G ? p.syndromes + (size_t)i * p.T * G + lane : nullptr;       // the lane's cell of round 0
    u8* hid = p.hidden + (size_t)i * d2 + (lane < d2 ? lane : 0);
    u8* triv = p.trivial + i;
    STREAM_IN_VGPR(syn); STREAM_IN_VGPR(hid); STREAM_IN_VGPR(triv);
    const StreamPtrs P = stream_ptrs((size_t)i, d2, lane, p.frame, p.weight, p.n_defects, p.rounds);
    StreamOut o;
    stream_windows<Closed>(p.c0, p.c1, p.T, p.window, p.commit, smem, lane, [&](int j, bool last) -> u64 {
        u32 w[4];                                                  // eval_sample_kernel's round, round counter j
        philox4x32_10((u32)j, 0u, id, (u32)lane, seed0, seed1, w);
        const bool hit = (u64)w[0] < Tq;
        const int typ = model == DQ_MODEL_X ? 1 : 1 + (int)__umulhi(w[1], 3u);
        const bool zhit = (u64)w[1] < Tq;
        const u64 ex = __ballot(model == DQ_MODEL_IIDXZ ? hit : hit && typ != 3);
        const u64 ez = __ballot(model == DQ_MODEL_IIDXZ ? zhit : hit && typ != 1);
        const u64 flips = Closed && last ? 0ull : __ballot((u64)w[2] < Tm);        // (closed: the last round is read without error, its data errors land)
        xmask ^= ex;
        zmask ^= ez;
        const u64 tw = __ballot(__popcll(((xmask & selx) | (zmask & ~selx)) & sq) & 1);
        const u64 v = tw ^ flips;
        summed |= v;
        if (syn) syn[(size_t)j * G] = (u8)((u32)(v >> (sidx & 63)) & cell_ok);
        const u64 cur = __ballot(((u32)(v >> (my_bit & 63)) & node_ok) != 0);
        const u64 D = cur ^ prev;
        prev = cur;
        return D;
    }, o);
    if (P.has_cell) {
        const int x = (int)((xmask >> lane) & 1), z = (int)((zmask >> lane) & 1);
        *hid = (u8)(x ? (z ? 2 : 1) : (z ? 3 : 0));
    }
    if (lane == 0) *triv = (u8)(summed == 0);
    stream_store(o, P, lane);
}

dq_status stream_check(const dq_decode_eval* V, int n, int T, int commit, const int32_t* weight_dev, const int32_t* n_defects_dev, const int32_t* rounds_dev,
                       const char* who) {
    DQ_REQUIRE(n >= 1 && n <= V->max_volumes, DQ_ERR_INVALID, "%s: n = %d outside 1..max_volumes %d", who, n, V->max_volumes);
    DQ_REQUIRE(T >= 1 && T <= STREAM_MAX_ROUNDS, DQ_ERR_INVALID, "%s: T = %d outside 1..%d", who, T, STREAM_MAX_ROUNDS);
    DQ_REQUIRE(((reinterpret_cast<uintptr_t>(weight_dev) | reinterpret_cast<uintptr_t>(n_defects_dev) | reinterpret_cast<uintptr_t>(rounds_dev)) & 3) == 0,
               DQ_ERR_INVALID, "%s: weight_dev, n_defects_dev and rounds_dev must be 4-byte aligned", who);
    DQ_REQUIRE(V->d <= 7 && V->depth >= 1 && V->depth <= UF_MAX_DEPTH, DQ_ERR_UNSUPPORTED, "%s: d = %d, window (volume_depth) = %d: union-find covers d <= 7, window <= %d",
               who, V->d, V->depth, UF_MAX_DEPTH);
    DQ_REQUIRE(commit >= 1 && commit <= V->depth, DQ_ERR_INVALID, "%s: commit = %d outside 1..window %d", who, commit, V->depth);
    return DQ_OK;
}

// The open and the closed entry points: one body, `who` names the caller in the messages.
dq_status stream_decode(bool closed, const char* who, dq_decode_eval* V, const uint8_t* syndromes_dev, int n, int T, int commit, uint8_t* frame_dev, int32_t* weight_dev,
                        int32_t* n_defects_dev, int32_t* rounds_dev, void* stream) {
    DQ_REQUIRE(V && syndromes_dev && frame_dev, DQ_ERR_INVALID, "%s: null argument", who);
    dq_status rc = stream_check(V, n, T, commit, weight_dev, n_defects_dev, rounds_dev, who);
    if (rc != DQ_OK) return rc;
    rc = match_st_tables(V);
    if (rc != DQ_OK) return rc;
    const MatchStTables* M = V->match_st;
    auto* kernel = closed ? stream_uf_kernel<true> : stream_uf_kernel<false>;
    kernel<<<n, 64, 0, (hipStream_t)stream>>>(M->uf[0], M->uf[1], M->cell, syndromes_dev, n, V->d, T, V->depth, commit, frame_dev, weight_dev, n_defects_dev, rounds_dev);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

dq_status stream_run(bool closed, const char* who, dq_decode_eval* V, const dq_env* env, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys,
                     double p_meas, const double* p_phys_each, const double* p_meas_each, uint8_t* hidden_dev, uint8_t* trivial_dev, uint8_t* frame_dev,
                     int32_t* weight_dev, int32_t* n_defects_dev, int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream) {
    DQ_REQUIRE(V && env && seed && hidden_dev && trivial_dev && frame_dev, DQ_ERR_INVALID, "%s: null argument", who);
    dq_status rc = stream_check(V, n, T, commit, weight_dev, n_defects_dev, rounds_dev, who);
    if (rc != DQ_OK) return rc;
    DQ_REQUIRE((p_phys_each != nullptr) == (p_meas_each != nullptr), DQ_ERR_INVALID, "%s: per-stream rates come as a pair of arrays", who);
    EnvRefereeView R;
    rc = env_referee_view(env, false, &R);
    if (rc != DQ_OK) return rc;
    // the lattice without the depth (dq_decode_verdict's check): the stream's length is T, the handle's volume_depth is the window
    DQ_REQUIRE(R.d == V->d && R.model == V->model && (R.model == DQ_MODEL_X || (R.use_Y != 0) == (V->use_Y != 0)), DQ_ERR_INVALID,
               "%s: the environment's lattice (d = %d, model %d, use_Y = %d) is not the decoder's (d = %d, model %d, use_Y = %d)", who, R.d, R.model, R.use_Y, V->d,
               V->model, V->use_Y);
    rc = match_st_tables(V);
    if (rc != DQ_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    StreamRunArgs a;
    memset(&a, 0, sizeof(a));
    if (p_phys_each) {
        rc = dq_rate_table_upload(V->rates, n, p_phys_each, p_meas_each, st);
        if (rc != DQ_OK) return rc;
        a.T_each = V->rates.dev;
    } else {
        DQ_REQUIRE(p_phys >= 0.0 && p_phys <= 1.0 && p_meas >= 0.0 && p_meas <= 1.0, DQ_ERR_INVALID, "%s: rates must be in [0,1]", who);
        a.T_phys = dq_rate_threshold(p_phys); a.T_meas = dq_rate_threshold(p_meas);
    }
    const MatchStTables* M = V->match_st;
    a.tab = R.tab; a.c0 = M->uf[0]; a.c1 = M->uf[1]; a.stab = M->stab;
    a.n = n; a.d = R.d; a.d2 = R.d * R.d; a.n_stab = R.n_stab; a.G = (R.d + 1) * (R.d + 1); a.model = R.model; a.T = T; a.window = V->depth; a.commit = commit;
    a.env_id_base = env_id_base; a.seed0 = seed[0]; a.seed1 = seed[1];
    a.hidden = hidden_dev; a.trivial = trivial_dev; a.frame = frame_dev; a.weight = weight_dev; a.n_defects = n_defects_dev; a.rounds = rounds_dev;
    a.syndromes = syndromes_dev;
    if (closed) stream_run_uf_kernel<true><<<n, 64, 0, st>>>(a);
    else stream_run_uf_kernel<false><<<n, 64, 0, st>>>(a);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

}  // namespace

extern "C" {

dq_status dq_stream_decode_uf(dq_decode_eval* V, const uint8_t* syndromes_dev, int n, int T, int commit, uint8_t* frame_dev, int32_t* weight_dev,
                              int32_t* n_defects_dev, int32_t* rounds_dev, void* stream) {
    return stream_decode(false, "dq_stream_decode_uf", V, syndromes_dev, n, T, commit, frame_dev, weight_dev, n_defects_dev, rounds_dev, stream);
}

dq_status dq_stream_decode_uf_closed(dq_decode_eval* V, const uint8_t* syndromes_dev, int n, int T, int commit, uint8_t* frame_dev, int32_t* weight_dev,
                                     int32_t* n_defects_dev, int32_t* rounds_dev, void* stream) {
    return stream_decode(true, "dq_stream_decode_uf_closed", V, syndromes_dev, n, T, commit, frame_dev, weight_dev, n_defects_dev, rounds_dev, stream);
}

dq_status dq_stream_run_uf(dq_decode_eval* V, const dq_env* env, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys, double p_meas,
                           const double* p_phys_each, const double* p_meas_each, uint8_t* hidden_dev, uint8_t* trivial_dev, uint8_t* frame_dev, int32_t* weight_dev,
                           int32_t* n_defects_dev, int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream) {
    return stream_run(false, "dq_stream_run_uf", V, env, n, T, commit, env_id_base, seed, p_phys, p_meas, p_phys_each, p_meas_each, hidden_dev, trivial_dev, frame_dev,
                      weight_dev, n_defects_dev, rounds_dev, syndromes_dev, stream);
}

dq_status dq_stream_run_uf_closed(dq_decode_eval* V, const dq_env* env, int n, int T, int commit, uint32_t env_id_base, const uint32_t seed[2], double p_phys,
                                  double p_meas, const double* p_phys_each, const double* p_meas_each, uint8_t* hidden_dev, uint8_t* trivial_dev, uint8_t* frame_dev,
                                  int32_t* weight_dev, int32_t* n_defects_dev, int32_t* rounds_dev, uint8_t* syndromes_dev, void* stream) {
    return stream_run(true, "dq_stream_run_uf_closed", V, env, n, T, commit, env_id_base, seed, p_phys, p_meas, p_phys_each, p_meas_each, hidden_dev, trivial_dev,
                      frame_dev, weight_dev, n_defects_dev, rounds_dev, syndromes_dev, stream);
}

}  // extern "C"
