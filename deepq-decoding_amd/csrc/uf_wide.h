// What the translation units around uf_wide_dev.h's component decode share (uf_wide.hip: streams; env_wide_uf.hip: the wide environment's volumes): the
// handle behind include/deepq_hip.h's dq_wide_uf, the register pinning of the values that live across a decode, and everything that tells the three variants
// of a decode apart -- unit weights, weighted (DESIGN.md sections 23, 24), correlated (sections 25, 26):
//   UfwMode, UfwWeights, ufw_check_weights   the variant, its weights as the entry points get them, their validation on the host
//   ufw_with_mode                            the one switch from a runtime UfwMode to the kernel templates' flags (Weighted, Corr)
//   ufw_setup                                a workgroup's prologue: its own weights, clamped, the LDS layout and the offset of the correlated masks
//   ufw_window                               one window's components: two decodes, or the three correlated passes
#pragma once
#include <type_traits>
#include "uf_wide_dev.h"

#define UFW_NODE_SLOTS 128                                       // thread 128 c + j <-> node j of component c
// A uniform value that lives across the component decode is kept in a vector register: the decode needs the scalar ones, and four waves of at most 64 KiB of LDS
// have vector registers to spare (uf_stream.hip's STREAM_IN_VGPR).
#define UFW_IN_VGPR(x) asm volatile("" : "+v"(x))

enum UfwMode { UFW_UNIT = 0, UFW_WEIGHTED = 1, UFW_CORRELATED = 2 };

// The weights of a weighted or a correlated launch: one pair (w_space, w_time) or triple (w_space, w_time, w_corr) for all streams / lattices, or one per
// stream.  A kernel of these two modes takes its file's unweighted arguments with this struct behind them; the unit-weight kernels take the unweighted ones.
struct UfwWeights {
    const u8* each;             // != NULL: stream i's bytes [s i] .. [s i + s - 1], s = 2 (weighted) or 3 (correlated); the uniform values are not read
    int w_space, w_time, w_corr;
};

// The correlated kernels' dynamic LDS is the layout's with the two masks behind it.
static inline int ufw_lds_bytes(UfwMode mode, int layout_bytes, int window) { return layout_bytes + (mode == UFW_CORRELATED ? ufw_mask_bytes(window) : 0); }

// What the weighted and the correlated entry points check before anything else: closed is a flag, the uniform pair lies in 1 .. UFW_MAX_WEIGHT, the uniform
// w_corr in 1 .. w_space.  A per-stream array is the caller's to check; the kernel clamps it.  each_excuses: the environment's forms do not look at the uniform
// values when an array is given; the stream forms (false) reject an invalid uniform pair even then.
static inline dq_status ufw_check_weights(UfwMode mode, int closed, const UfwWeights& w, bool each_excuses, const char* who) {
    DQ_REQUIRE(closed == 0 || closed == 1, DQ_ERR_INVALID, "%s: closed = %d is not 0 or 1", who, closed);
    if (each_excuses && w.each != nullptr) return DQ_OK;
    DQ_REQUIRE(w.w_space >= 1 && w.w_space <= UFW_MAX_WEIGHT && w.w_time >= 1 && w.w_time <= UFW_MAX_WEIGHT, DQ_ERR_INVALID,
               "%s: weights (%d, %d) outside 1..%d", who, w.w_space, w.w_time, UFW_MAX_WEIGHT);
    DQ_REQUIRE(mode != UFW_CORRELATED || (w.w_corr >= 1 && w.w_corr <= w.w_space), DQ_ERR_INVALID, "%s: w_corr = %d outside 1..w_space = %d", who, w.w_corr,
               w.w_space);
    return DQ_OK;
}

// f(Weighted, Corr) with the mode's two template flags as std::bool_constant values.  Each file maps (its own flags, mode) to a kernel instantiation in one
// function built on this, and both its launches and its hipFuncSetAttribute loop go through that function: what can be launched has its LDS limit raised.
template <class F>
static inline void ufw_with_mode(UfwMode mode, F&& f) {
    if (mode == UFW_CORRELATED) f(std::true_type{}, std::true_type{});
    else if (mode == UFW_WEIGHTED) f(std::true_type{}, std::false_type{});
    else f(std::false_type{}, std::false_type{});
}

#ifdef __HIPCC__
static __device__ __forceinline__ void ufw_layout_in_vgpr(UfwLayout& L) {
    UFW_IN_VGPR(L.o_frame); UFW_IN_VGPR(L.o_carry); UFW_IN_VGPR(L.o_acc); UFW_IN_VGPR(L.o_ring); UFW_IN_VGPR(L.o_label); UFW_IN_VGPR(L.o_par);
    UFW_IN_VGPR(L.o_parent); UFW_IN_VGPR(L.o_level); UFW_IN_VGPR(L.o_g); UFW_IN_VGPR(L.o_ex); UFW_IN_VGPR(L.o_ez); UFW_IN_VGPR(L.o_v);
}

// What a workgroup computes once in front of its decode: its own weights (1 where the variant has none), the layout of its dynamic LDS for (n, d2, window) and,
// for the correlated kernels, the byte offset of the two masks behind the layout.  Every thread reads the same bytes of w.each, so the weights are
// workgroup-uniform.  The pair is clamped to 1 .. UFW_MAX_WEIGHT, w_corr to 1 .. w_space: a bad byte of a per-stream array cannot overrun the growth byte.
struct UfwSetup {
    UfwLayout L;
    int w_space, w_time, w_corr, o_mask;
};

template <bool Weighted, bool Corr, class Args>
static __device__ __forceinline__ UfwSetup ufw_setup(const Args& p, size_t i, int n, int d2, int window) {
    UfwSetup S;
    S.w_space = S.w_time = S.w_corr = 1; S.o_mask = 0;
    if constexpr (Weighted) {
        constexpr int stride = Corr ? 3 : 2;
        const UfwWeights& w = p.w;
        S.w_space = w.w_space; S.w_time = w.w_time;
        if constexpr (Corr) S.w_corr = w.w_corr;
        if (w.each != nullptr) {
            S.w_space = w.each[stride * i]; S.w_time = w.each[stride * i + 1];
            if constexpr (Corr) S.w_corr = w.each[stride * i + 2];
        }
        S.w_space = min(max(S.w_space, 1), UFW_MAX_WEIGHT); S.w_time = min(max(S.w_time, 1), UFW_MAX_WEIGHT);
        if constexpr (Corr) S.w_corr = min(max(S.w_corr, 1), S.w_space);
        UFW_IN_VGPR(S.w_space); UFW_IN_VGPR(S.w_time);
        if constexpr (Corr) UFW_IN_VGPR(S.w_corr);
    }
    S.L = ufw_layout(n, d2, window);
    if constexpr (Corr) { S.o_mask = S.L.bytes; UFW_IN_VGPR(S.o_mask); }
    ufw_layout_in_vgpr(S.L);
    return S;
}

// The head of the layout in the workgroup's LDS: the two frames, the two carries, the eight accumulator words and the ring of defect rows.
struct UfwHead {
    u32 *s_frame, *s_carry;
    int* s_acc;
    u32* s_ring;
};

static __device__ __forceinline__ UfwHead ufw_head(u8* smem, const UfwLayout& L) {
    return UfwHead{reinterpret_cast<u32*>(smem + L.o_frame), reinterpret_cast<u32*>(smem + L.o_carry), reinterpret_cast<int*>(smem + L.o_acc),
                   reinterpret_cast<u32*>(smem + L.o_ring)};
}

// The graph of a lattice without a window's depth, and the endpoint tables of its two components, in vector registers.
static __device__ __forceinline__ UfwGraph ufw_graph_in_vgpr(int n, int d2) {
    UfwGraph G;
    G.n = n; G.d2 = d2; G.per_round = d2 + n;
    G.mag_n = ufw_magic(G.n); G.mag_pr = ufw_magic(G.per_round);
    UFW_IN_VGPR(G.n); UFW_IN_VGPR(G.d2); UFW_IN_VGPR(G.per_round); UFW_IN_VGPR(G.mag_n); UFW_IN_VGPR(G.mag_pr);
    return G;
}

struct UfwEnds {
    const u8 *eu0, *ev0, *eu1, *ev1;
};

static __device__ __forceinline__ UfwEnds ufw_ends_in_vgpr(const UfwComp& c0, const UfwComp& c1) {
    UfwEnds E = {c0.eu, c0.ev, c1.eu, c1.ev};
    UFW_IN_VGPR(E.eu0); UFW_IN_VGPR(E.ev0); UFW_IN_VGPR(E.eu1); UFW_IN_VGPR(E.ev1);
    return E;
}

// One window's components by the whole workgroup: the rows of component c are the ring's u32 [G.depth][4] at row_stride c, its frame, carry, weight and growth
// rounds the layout's words of c, and commit / final are ufw_component's.  n_comp: 2, or 1 where component 1's frame is not asked for (workgroup-uniform).
// s_event: the o_acc word that the weighted growth's event reduction may use.
// Unit and weighted: component 0, then component 1.  Corr: three decodes -- component 0 dry, which only leaves mask A of its
// correction's space edges; component 1 with w_corr on A, committed, leaving mask B; component 0 again with w_corr on B, committed.  The masks u32 [2][..][8]
// lie at S.o_mask, mask_stride = 2 row_stride words apart.  Two workgroup-uniform skips: without a defect of component 1 in the window nobody reads A and the
// dry pass is left out; with n_comp = 1 nobody writes B, and the last pass alone runs under w_corr = w_space, where no bit of B tells: the weighted decode.
template <bool Closed, bool Weighted, bool Corr>
static __device__ __forceinline__ void ufw_window(UfwGraph& G, const UfwEnds& E, u8* smem, const UfwSetup& S, const UfwHead& H, int tid, int row_stride,
                                                  int commit, bool final, int n_comp, int* s_event) {
    const UfwLayout& L = S.L;
    u32 *s_frame = H.s_frame, *s_carry = H.s_carry, *s_ring = H.s_ring;
    int* s_acc = H.s_acc;
    if constexpr (Corr) {
        u32* s_mask = reinterpret_cast<u32*>(smem + S.o_mask);     // A, B
        int mask_stride = row_stride * (UFW_FRAME_WORDS / UFW_ROW_WORDS);
        int w_corr = S.w_corr, pass = 2;
        if (n_comp < 2) w_corr = S.w_space;
        else pass = __syncthreads_or(tid < G.depth * UFW_ROW_WORDS && s_ring[row_stride + tid] != 0) ? 0 : 1;
        UFW_IN_VGPR(mask_stride); UFW_IN_VGPR(pass);
        for (; pass < 3; ++pass) {                                 // components 0, 1, 0
            const int c = pass & 1;
            int dry = pass == 0;
            UFW_IN_VGPR(dry);
            G.eu = c ? E.eu1 : E.eu0; G.ev = c ? E.ev1 : E.ev0;
            // pass 0 reads B, which nobody has written for this window, under w_corr = w_space: every space edge weighs w_space
            ufw_component<Closed, true, true>(G, s_ring + c * row_stride, smem, L, tid, commit, final, s_frame + c * UFW_FRAME_WORDS, s_carry + c * UFW_ROW_WORDS,
                                              s_acc + c, s_acc + 4 + c, S.w_space, S.w_time, s_event, pass ? w_corr : S.w_space,
                                              s_mask + (c ? 0 : mask_stride), s_mask + (c ? mask_stride : 0), dry);
        }
    } else {
        for (int c = 0; c < n_comp; ++c) {                         // (Weighted = false: ufw_component does not read the last three arguments)
            G.eu = c ? E.eu1 : E.eu0; G.ev = c ? E.ev1 : E.ev0;
            ufw_component<Closed, Weighted>(G, s_ring + c * row_stride, smem, L, tid, commit, final, s_frame + c * UFW_FRAME_WORDS, s_carry + c * UFW_ROW_WORDS,
                                            s_acc + c, s_acc + 4 + c, S.w_space, S.w_time, s_event);
        }
    }
}

// A round's two defect rows from the current and the previous syndrome bit of thread 128 c + j's node: a wave's ballot is words 2 (wave & 1), + 1 of component
// wave >> 1's row.  nd: the wave's count of its component's defects.
static __device__ __forceinline__ void wide_rows(int cur, int& prev, int tid, u32* row0, u32* row1, int& nd) {
    const u64 D = __ballot(cur != prev);
    prev = cur;
    nd += __popcll(D);
    if ((tid & 63) == 0) {
        u32* row = (tid >> 7) ? row1 : row0;
        const int w = ((tid >> 6) & 1) * 2;
        row[w] = (u32)D; row[w + 1] = (u32)(D >> 32);
    }
}
#endif

struct dq_wide_uf {
    int d, model, window, max_streams, n, d2, n_stab, G, lds;
    u8* blob;                   // the tables below, one allocation
    const u8 *ends;             // [2][2][256] UfwComp eu / ev per component
    const u8 *node_cell;        // [2][128] node -> cell a (d + 1) + b of the syndrome grid, 255: no node
    const u8 *node_stab;        // [2][128] node -> stabilizer in measurement order, 255: no node
    const u8 *cell_stab;        // [256] cell -> stabilizer, 255: a dead corner
    const u8 *stab_q;           // [256][4] stabilizer -> its qubits, 255: none
    const u8 *stab_isx;         // [256] 1: the stabilizer reads the X plane (type 3)
    DqRateTable rates;
};
