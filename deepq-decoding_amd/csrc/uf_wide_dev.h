// Device side of the wide union-find stream decoder (uf_wide.hip): section 16's component decode (uf_dev.h) inside section 17's
// window schedule (uf_stream.hip), unchanged as an algorithm, for any odd d in 3 .. 15 and a window of up to 32 rounds -- one Pauli component of one window by
// one WORKGROUP of UFW_THREADS threads (four waves) instead of one wavefront.
//
// Graph, unit weights, n = (d^2 - 1) / 2 nodes per round: node (u, t) = t n + u, B = depth n; edge ids t (d^2 + n) + k, k = q < d^2 the space edge of qubit q,
// k = d^2 + u the time edge (u, t) -- (u, t + 1), in the last round (u, t) -- B.  Growth in synchronous rounds with g in {0, 1, 2}, min-labels (0 = holds B,
// else lowest node + 1), peeling by levels with the lowest-edge-id parent: uf_dev.h's text applies word for word.  What differs is the shape:
//   * the phases are separated by workgroup barriers, and every loop exit is decided by a barrier that reduces the predicate over the workgroup
//     (__syncthreads_or) or by a value every thread computes alike from the kernel's arguments: no wave can leave a loop its siblings are still in;
//   * the edges' ends are not stored: they follow from (t, k) and the component's endpoint table (UfwComp: d^2 bytes per end, read through the cache);
//   * a defect row and the carry are UFW_ROW_WORDS x 32 bits (n <= 112), the frame of a component UFW_FRAME_WORDS x 32 bits (d^2 <= 225): LDS words,
//     accumulated with LDS atomics;
//   * the LDS is dynamic and sized from the call's (d, window) by ufw_layout, the same function on the host and on the device.
// Every loop bound is a constant of (d, window, T, commit), which the host validates.  No scratch pool, no lock, no loop that waits on another workgroup.
//
// Weighted growth (ufw_component<Closed, true>): an edge of weight w is full at g = 2 w, w = w_space for k < d^2 and w_time for
// k >= d^2, both in 1 .. UFW_MAX_WEIGHT, one pair per stream.  The growth byte then holds g in bits 0 .. 4, the edge's increment of the running event in bits
// 5 .. 6 and "full" in bit 7; the layout is the unweighted one.  Growth jumps from event to event: the workgroup reduces the number of unit steps until the
// next edge fills (an LDS atomic minimum into a spare word of o_acc), every growing edge gains that many increments, and `rounds` counts the unit steps.
//
// Correlated decode (ufw_component<Closed, true, true>): the weight of a space edge is per edge -- w_corr where the edge's bit of a mask
// u32 [depth][UFW_FRAME_WORDS] is set, else w_space -- and the peeling sets the bit of every space edge of the correction, committed or not, in a second
// mask.  The two masks are a tail of 2 x window x UFW_FRAME_WORDS words behind ufw_layout's bytes (ufw_mask_bytes), for the correlated kernels only.
#pragma once
#include "common.h"

#define UFW_THREADS 256
#define UFW_MAX_D 15
#define UFW_MAX_WINDOW 32
#define UFW_ROW_WORDS 4                                          // 32-bit words of a defect row / a carry: n <= 112
#define UFW_FRAME_WORDS 8                                        // 32-bit words of a component's frame: d^2 <= 225
#define UFW_NONE 0xffffffffu
#define UFW_NOLEVEL 0xffffu
#define UFW_MAX_WEIGHT 15                                        // 2 w <= 30 fits the five growth bits
#define UFW_G_MASK 0x1fu
#define UFW_INC_SHIFT 5
#define UFW_FULL 0x80u
#define UFW_NO_EVENT 0x7fffffff

struct UfwComp {
    const u8* eu;           // [d^2] qubit -> its first plaquette of the component (node index)
    const u8* ev;           // [d^2] ... its second one, 255: none (the edge goes to B)
};

// Byte offsets of a workgroup's dynamic LDS for (n, d2, window).  The head is fixed, the graph arrays follow.
struct UfwLayout {
    int o_frame, o_carry, o_acc, o_ring, o_label, o_par, o_parent, o_level, o_g, o_ex, o_ez, o_v, bytes;
};

static __host__ __device__ inline UfwLayout ufw_layout(int n, int d2, int window) {
    UfwLayout L;
    const int NN = window * n + 1, NE = window * (d2 + n);
    int o = 0;
    L.o_frame = o; o += 2 * UFW_FRAME_WORDS * 4;                 // u32 [2][8] committed space edges per component
    L.o_carry = o; o += 2 * UFW_ROW_WORDS * 4;                   // u32 [2][4] the carry into the next window
    L.o_acc = o; o += 8 * 4;                                     // int [2] weight, [2] defects, [2] growth rounds, [1] steps to the next event (weighted), [1] spare
    L.o_ring = o; o += 2 * window * UFW_ROW_WORDS * 4;           // u32 [2][window][4] defect rows of the window
    L.o_label = o; o += 4 * NN;                                  // u32 [NN] cluster label
    L.o_par = o; o += 4 * NN;                                    // u32 [NN] defect parity per label; then subtree parity per node
    L.o_parent = o; o += 4 * NN;                                 // u32 [NN] parent edge
    L.o_level = o; o += (2 * NN + 3) & ~3;                       // u16 [NN]
    L.o_g = o; o += (NE + 3) & ~3;                               // u8 [NE] growth
    L.o_ex = o; o += 256;                                        // u8 [256] the sampler's X plane / the verdict's
    L.o_ez = o; o += 256;                                        // u8 [256] ... Z plane
    L.o_v = o; o += 256;                                         // u8 [256] the round's faulty syndrome bits, measurement order
    L.bytes = o;
    return L;
}

// The correlated kernels' tail behind ufw_layout(...).bytes: two masks u32 [window][UFW_FRAME_WORDS], one read while the other is written.
static __host__ __device__ inline int ufw_mask_bytes(int window) { return 2 * window * UFW_FRAME_WORDS * 4; }

#ifdef __HIPCC__

// x / p for x < 2^32 / p by one multiply: m = floor(2^32 / p) + 1
static __device__ __forceinline__ u32 ufw_magic(int p) { return 0xffffffffu / (u32)p + 1u; }
static __device__ __forceinline__ int ufw_div(int x, u32 magic) { return (int)__umulhi((u32)x, magic); }

struct UfwGraph {
    int n, d2, per_round, depth, B, NN, NE;
    u32 mag_n, mag_pr;
    const u8* eu;
    const u8* ev;
};

static __device__ __forceinline__ void ufw_ends(const UfwGraph& G, int e, int& a, int& b, int& t, int& k) {
    t = ufw_div(e, G.mag_pr);
    k = e - t * G.per_round;
    if (k < G.d2) {
        const int u = G.eu[k], v = G.ev[k];
        a = u == 255 ? G.B : t * G.n + u;
        b = (u == 255 || v == 255) ? G.B : t * G.n + v;
    } else {
        a = t * G.n + (k - G.d2);
        b = t + 1 < G.depth ? a + G.n : G.B;
    }
}

// The weight of edge (t, k): w_time for a time edge, w_space for a space edge -- with Corr, w_corr where the mask u32 [depth][UFW_FRAME_WORDS] has the edge's bit.
template <bool Corr>
static __device__ __forceinline__ int ufw_weight(int t, int k, int d2, int w_space, int w_time, int w_corr, volatile const u32* mask) {
    if constexpr (Corr) {
        if (k >= d2) return w_time;
        return (mask[t * UFW_FRAME_WORDS + (k >> 5)] >> (k & 31)) & 1u ? w_corr : w_space;
    } else {
        return k < d2 ? w_space : w_time;
    }
}

// One component of one window by the whole workgroup; every thread calls it with the same arguments.  dw: the component's rows u32 [depth][4] in LDS.
// Unless `final`, only the edges of rounds t < commit count; a committed space edge XORs its qubit into s_frame [8], a committed edge adds 1 to *s_weight, the
// time edges of round commit - 1 set their bit of s_carry [4] (zero on entry).  The growth rounds made are added to *s_rounds.
// Closed (a stream that ends on a round of perfect measurements): in a `final` window the time edges of the last round do not exist.
// They are the last n edge ids, and the growth loop stops in front of them: never grown, they are never full, so no label crosses them, no level reaches
// across them and they are never in the correction.
// Weighted: w_space / w_time in 1 .. UFW_MAX_WEIGHT (the caller clamps), s_event the LDS word of the event reduction; a committed edge adds its weight to
// *s_weight, *s_rounds counts unit growth steps.  With Weighted = false the three arguments are not read and the code is the unit-weight one.
// Corr (with Weighted): the space edge (t, k) weighs w_corr where bit k of mask_r [t][8] is set; mask_w [depth][8] is zeroed on entry, in front of the early
// return, and receives the bit of every space edge of the correction, whatever its round.  dry (workgroup-uniform): nothing is committed -- frame, carry, weight
// and rounds stay as they are.  With Corr = false the four arguments are not read and the code is the weighted one.
// uf_wide.h's ufw_window is the one caller: it passes every argument whatever the flags.
template <bool Closed = false, bool Weighted = false, bool Corr = false>
static __device__ __forceinline__ void ufw_component(const UfwGraph& G, const u32* dw, u8* __restrict__ s, const UfwLayout& L, int tid, int commit, bool final,
                                                     u32* s_frame, u32* s_carry, int* s_weight, int* s_rounds, int w_space = 1, int w_time = 1,
                                                     int* s_event = nullptr, int w_corr = 1, const u32* mask_r = nullptr, u32* mask_w = nullptr,
                                                     int dry = 0) {
    static_assert(Weighted || !Corr, "the correlated decode is a weighted one");
    u32* s_label = reinterpret_cast<u32*>(s + L.o_label);
    u32* s_par = reinterpret_cast<u32*>(s + L.o_par);
    u32* s_parent = reinterpret_cast<u32*>(s + L.o_parent);
    volatile u32* v_label = s_label;
    volatile u32* v_par = s_par;
    volatile u32* v_parent = s_parent;
    volatile uint16_t* s_level = reinterpret_cast<volatile uint16_t*>(s + L.o_level);
    volatile u8* s_g = s + L.o_g;
    volatile const u32* v_dw = dw;
    const int n = G.n, B = G.B, NN = G.NN, NE = G.NE;
    const int NE_grown = Closed && final ? NE - n : NE;
    const int d2 = G.d2;
    volatile const u32* v_mask = mask_r;
#define UFW_WEIGHT_OF(t, k) ufw_weight<Corr>(t, k, d2, w_space, w_time, w_corr, v_mask)
    if constexpr (Corr) {                                         // (depth <= UFW_MAX_WINDOW: one word per thread; the barrier below publishes it)
        if (tid < G.depth * UFW_FRAME_WORDS) mask_w[tid] = 0;
    }
    // nothing to correct: workgroup-uniform, the graph arrays untouched
    if (!__syncthreads_or(tid < G.depth * UFW_ROW_WORDS && v_dw[tid] != 0)) return;
    auto defect = [&](int x) -> u32 {
        if (x >= B) return 0u;
        const int t = ufw_div(x, G.mag_n), u = x - t * n;
        return (v_dw[t * UFW_ROW_WORDS + (u >> 5)] >> (u & 31)) & 1u;
    };
    for (int e = tid; e < NE; e += UFW_THREADS) s_g[e] = 0;
    for (int x = tid; x < NN; x += UFW_THREADS) v_label[x] = x == B ? 0u : (u32)x + 1u;
    __syncthreads();
    // ---- growth ---------------------------------------------------------------------------------------------------------------------------------
    int rounds = 0;
    if constexpr (!Weighted) {
        const int round_bound = 2 * NE;
        for (int r = 0; r <= round_bound; ++r) {
            for (int x = tid; x < NN; x += UFW_THREADS) v_par[x] = 0;
            __syncthreads();
            for (int x = tid; x < B; x += UFW_THREADS)
                if (defect(x)) __hip_atomic_fetch_xor(s_par + v_label[x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __syncthreads();
            bool any = false;
            for (int x = tid; x < B; x += UFW_THREADS) { const u32 l = v_label[x]; any |= l != 0 && (v_par[l] & 1u); }
            if (!__syncthreads_or(any) || r == round_bound) break;    // workgroup-uniform
            ++rounds;
            bool fresh = false;
            for (int e = tid; e < NE_grown; e += UFW_THREADS) {
                const int g0 = s_g[e];
                if (g0 == 2) continue;
                int a, b, t, k;
                ufw_ends(G, e, a, b, t, k);
                const u32 la = v_label[a], lb = v_label[b];
                const int inc = (int)(la != 0 && (v_par[la] & 1u)) + (int)(lb != 0 && (v_par[lb] & 1u));
                const int g1 = min(2, g0 + inc);
                if (g1 != g0) { s_g[e] = (u8)g1; fresh |= g1 == 2; }
            }
            if (!__syncthreads_or(fresh)) continue;               // workgroup-uniform: no new full edge, the clusters stand
            for (int pass = 0; pass < NN; ++pass) {               // (a label travels at least one edge per pass)
                bool changed = false;
                for (int e = tid; e < NE; e += UFW_THREADS) {
                    if (s_g[e] != 2) continue;
                    int a, b, t, k;
                    ufw_ends(G, e, a, b, t, k);
                    const u32 la = v_label[a], lb = v_label[b];
                    if (la != lb) {
                        const u32 m = la < lb ? la : lb;
                        __hip_atomic_fetch_min(s_label + (la < lb ? b : a), m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        changed = true;
                    }
                }
                if (!__syncthreads_or(changed)) break;            // workgroup-uniform
            }
        }
    } else {
        // One event per pass: the steps until the next edge fills are reduced over the workgroup, every growing edge gains that many increments, and at
        // least one edge fills.  So NE_grown + 1 passes cover any growth, a constant of the window's shape.
        volatile int* v_event = s_event;
        int events_left = NE_grown + 1;
        asm volatile("" : "+v"(events_left));                 // (uf_wide.h UFW_IN_VGPR: the scalar registers are the scarce ones)
        for (;; --events_left) {
            if (tid == 0) *v_event = UFW_NO_EVENT;                // (the previous pass read it in front of its last barriers)
            for (int x = tid; x < NN; x += UFW_THREADS) v_par[x] = 0;
            __syncthreads();
            for (int x = tid; x < B; x += UFW_THREADS)
                if (defect(x)) __hip_atomic_fetch_xor(s_par + v_label[x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __syncthreads();
            bool any = false;
            for (int x = tid; x < B; x += UFW_THREADS) { const u32 l = v_label[x]; any |= l != 0 && (v_par[l] & 1u); }
            if (!__syncthreads_or(any) || events_left == 0) break;    // workgroup-uniform
            int steps = UFW_NO_EVENT;
            for (int e = tid; e < NE_grown; e += UFW_THREADS) {
                const u32 g0 = s_g[e];
                if (g0 & UFW_FULL) continue;
                int a, b, t, k;
                ufw_ends(G, e, a, b, t, k);
                const u32 la = v_label[a], lb = v_label[b];
                const int inc = (int)(la != 0 && (v_par[la] & 1u)) + (int)(lb != 0 && (v_par[lb] & 1u));
                if (!inc) continue;
                const int left = 2 * UFW_WEIGHT_OF(t, k) - (int)g0;             // > 0: the edge is not full
                steps = min(steps, (left + inc - 1) >> (inc - 1));             // ceil(left / inc), inc in {1, 2}
                s_g[e] = (u8)(g0 | ((u32)inc << UFW_INC_SHIFT));
            }
            if (steps != UFW_NO_EVENT) __hip_atomic_fetch_min(s_event, steps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __syncthreads();
            const int jump = *v_event;                            // one word, written in front of the barrier: workgroup-uniform
            if (jump == UFW_NO_EVENT) break;                      // (an odd cluster without B always has a growing edge; were there none, nothing could change)
            rounds += jump;
            for (int e = tid; e < NE_grown; e += UFW_THREADS) {   // (thread and edge as above: an increment is read by the thread that wrote it)
                const u32 g0 = s_g[e];
                const int inc = (int)((g0 >> UFW_INC_SHIFT) & 3u);
                if (!inc) continue;
                const int t = ufw_div(e, G.mag_pr), k = e - t * G.per_round, cap = 2 * UFW_WEIGHT_OF(t, k);
                const int g1 = min(cap, (int)(g0 & UFW_G_MASK) + inc * jump);
                s_g[e] = (u8)(g1 == cap ? (u32)g1 | UFW_FULL : (u32)g1);
            }
            __syncthreads();
            for (int pass = 0; pass < NN; ++pass) {               // (a label travels at least one edge per pass)
                bool changed = false;
                for (int e = tid; e < NE; e += UFW_THREADS) {
                    if (!(s_g[e] & UFW_FULL)) continue;
                    int a, b, t, k;
                    ufw_ends(G, e, a, b, t, k);
                    const u32 la = v_label[a], lb = v_label[b];
                    if (la != lb) {
                        const u32 m = la < lb ? la : lb;
                        __hip_atomic_fetch_min(s_label + (la < lb ? b : a), m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        changed = true;
                    }
                }
                if (!__syncthreads_or(changed)) break;            // workgroup-uniform
            }
        }
    }
    // ---- peeling: levels and parent edges ---------------------------------------------------------------------------------------------------------
    for (int x = tid; x < NN; x += UFW_THREADS) {
        s_level[x] = (uint16_t)((x == B || v_label[x] == (u32)x + 1u) ? 0u : UFW_NOLEVEL);
        v_parent[x] = UFW_NONE;
        v_par[x] = defect(x);
    }
    __syncthreads();
    int deepest = 0;
    for (int lev = 1; lev < NN; ++lev) {
        for (int e = tid; e < NE; e += UFW_THREADS) {
            if (Weighted ? !(s_g[e] & UFW_FULL) : s_g[e] != 2) continue;
            int a, b, t, k;
            ufw_ends(G, e, a, b, t, k);
            const u32 va = s_level[a], vb = s_level[b];
            if (va == (u32)(lev - 1) && vb == UFW_NOLEVEL) __hip_atomic_fetch_min(s_parent + b, (u32)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else if (vb == (u32)(lev - 1) && va == UFW_NOLEVEL) __hip_atomic_fetch_min(s_parent + a, (u32)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        bool reached = false;
        for (int x = tid; x < B; x += UFW_THREADS)
            if (s_level[x] == UFW_NOLEVEL && v_parent[x] != UFW_NONE) { s_level[x] = (uint16_t)lev; reached = true; }
        if (!__syncthreads_or(reached)) break;                    // workgroup-uniform
        deepest = lev;
    }
    // ---- peeling: from the deepest level down ---------------------------------------------------------------------------------------------------------
    int w = 0;
    for (int lev = deepest; lev >= 1; --lev) {
        for (int x = tid; x < B; x += UFW_THREADS) {
            if (s_level[x] != (u32)lev || !(v_par[x] & 1u)) continue;
            const int e = (int)v_parent[x];
            int a, b, t, k;
            ufw_ends(G, e, a, b, t, k);
            __hip_atomic_fetch_xor(s_par + (a == x ? b : a), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if constexpr (Corr) {
                if (k < G.d2) __hip_atomic_fetch_or(mask_w + t * UFW_FRAME_WORDS + (k >> 5), 1u << (k & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (dry) continue;
            }
            if (!final) {                                         // (an edge is in the correction once: its lower end has one parent edge)
                if (t >= commit) continue;
                if (k >= G.d2 && t == commit - 1) {
                    const int u = k - G.d2;
                    __hip_atomic_fetch_or(s_carry + (u >> 5), 1u << (u & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            w += Weighted ? UFW_WEIGHT_OF(t, k) : 1;
            if (k < G.d2) __hip_atomic_fetch_xor(s_frame + (k >> 5), 1u << (k & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
    }
    if (w) __hip_atomic_fetch_add(s_weight, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (tid == 0 && !(Corr && dry)) *s_rounds += rounds;
    __syncthreads();                                              // every thread is through with the graph arrays before the next component reuses them
#undef UFW_WEIGHT_OF
}

#endif  // __HIPCC__
