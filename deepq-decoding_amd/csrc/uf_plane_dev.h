// Device side of the union-find referee: section 20's closed union-find decode on a one-round window -- code-capacity decoding, a perfect
// syndrome in, a homology class out -- for one Pauli component of any odd d in 3 .. 15 by ONE wavefront.  Shared by env_big.hip (the referee inside the wide
// environment's step), verdict_wide.hip (the refereed verdict) and uf_plane.hip (dq_uf_referee_decode).
//
// Graph: the n = (d^2 - 1) / 2 plaquettes of the component are the nodes, in the look-up and matching referee's index order (lattice_host.h `typed`), B = n is the
// boundary; only the d^2 space edges exist and edge id = qubit id (the one-round window's time edges are not alive when the window is closed: they never grow, are
// never full and never in the correction, so they are not built).  Growth in synchronous rounds with g in {0, 1, 2}, min-labels (0 = holds B, else lowest node + 1),
// peeling by breadth-first levels with the lowest-edge-id parent: uf_dev.h's text applies word for word, and so does its match_wave_sync discipline.  The class is
// the parity of the logical bits of the correction's qubits: qubit q = x d + y counts for component 0 when y = 0, for component 1 when x = 0 (FL:312-317).
//
// Shape: lane l owns the edges l, l + 64, l + 128, l + 192 (d^2 <= 225) and the nodes l, l + 64 (n <= 112).  An edge lives in one register of its lane:
//   bits 0 .. 7 one end, 8 .. 15 the other (B where the qubit has one plaquette of the component; an edge id >= d^2 has both ends at B: label 0 is never active, so
//   it never grows), bit 16 the qubit's logical bit, bits 24 .. 25 the growth.
// What lanes hand to each other goes through the wave's own LDS, UFP_LDS = 1520 bytes:
//   label  u32 [116]  at    0   cluster label
//   par    u32 [116]  at  464   defect parity per label; then subtree parity per node
//   parent u32 [116]  at  928   parent edge e << 9 | logical bit << 8 | the node at the edge's other end (the minimum over this word is the minimum over e: the other
//                               end is a function of (e, node)); the peeling then needs no edge that another lane holds
//   level  u8  [128]  at 1392   breadth-first level, 255: none (a level is below n + 1 <= 113)
// Every loop bound is a constant of (n, d^2); every exit is wave-uniform and taken from the wave's own data; nothing spins, nothing is shared between waves; no
// scratch pool, no lock, no fallback: the answer is the rule's for any number of defects.
#pragma once
#include "match_dev.h"                                           // match_wave_sync

#define UFP_MAX_NODES 112
#define UFP_MAX_EDGES 225
#define UFP_SLOTS 116                                            // n + 1 <= 113, padded
#define UFP_O_LABEL 0
#define UFP_O_PAR (UFP_O_LABEL + 4 * UFP_SLOTS)
#define UFP_O_PARENT (UFP_O_PAR + 4 * UFP_SLOTS)
#define UFP_O_LEVEL (UFP_O_PARENT + 4 * UFP_SLOTS)
#define UFP_LDS (UFP_O_LEVEL + 128)
#define UFP_NONE 0xffffffffu
#define UFP_NOLEVEL 0xffu
#define UFP_G_SHIFT 24

struct UfPlane {
    const u8* eu;           // [d^2] qubit -> its first plaquette of the component (node index)
    const u8* ev;           // [d^2] ... its second one, 255: none (the edge goes to B)
    int n, d, comp;         // nodes; the distance; 0: the X plane's component (logical bit on column 0), 1: the Z plane's (row 0)
};

// Class predicted for the defects `d0 | d1 << 64` (bit i = i-th plaquette of the component in row-major order: match_classify's convention).  All lanes of the wave
// call it with the same arguments; the result is wave-uniform.  `s` = UFP_LDS bytes of LDS owned by this wave.  The empty syndrome gives class 0 and leaves `s`
// untouched.
static __device__ __forceinline__ int uf_plane_classify(const UfPlane& G, u64 d0, u64 d1, u8* __restrict__ s, int lane) {
    if ((d0 | d1) == 0) return 0;                                 // wave-uniform
    u32* s_label = reinterpret_cast<u32*>(s + UFP_O_LABEL);
    u32* s_par = reinterpret_cast<u32*>(s + UFP_O_PAR);
    u32* s_parent = reinterpret_cast<u32*>(s + UFP_O_PARENT);
    volatile u32* v_label = s_label;
    volatile u32* v_par = s_par;
    volatile u32* v_parent = s_parent;
    volatile u8* s_level = s + UFP_O_LEVEL;
    const int n = min(G.n, UFP_MAX_NODES), d2 = min(G.d * G.d, UFP_MAX_EDGES), B = n, NN = n + 1;
    const u32 mag_d = 0xffffffffu / (u32)G.d + 1u;                // e / d for e < 2^32 / d by one multiply
    auto defect = [&](int x) -> u32 { return x < n ? (u32)(((x < 64 ? d0 : d1) >> (x & 63)) & 1ull) : 0u; };
    // ---- edges and singleton clusters --------------------------------------------------------------------------------------------------------
    u32 ed[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = lane + 64 * k;
        u32 a = (u32)B, b = (u32)B, lg = 0;
        if (e < d2) {
            const u32 u = G.eu[e], v = G.ev[e];
            a = u < (u32)n ? u : (u32)B;
            b = (u < (u32)n && v < (u32)n) ? v : (u32)B;
            const int row = (int)__umulhi((u32)e, mag_d);
            lg = G.comp ? row == 0 : e - row * G.d == 0;
        }
        ed[k] = a | b << 8 | lg << 16;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) { const int x = lane + 64 * j; if (x < NN) v_label[x] = x == B ? 0u : (u32)x + 1u; }
    match_wave_sync();                                            // (also orders this call's writes after a previous call's reads of `s`)
    // ---- growth ---------------------------------------------------------------------------------------------------------------------------------
    const int round_bound = 2 * d2;                               // (a round with an active cluster grows an edge, and the growths sum to at most 2 d^2)
    for (int r = 0; r <= round_bound; ++r) {
#pragma unroll
        for (int j = 0; j < 2; ++j) { const int x = lane + 64 * j; if (x < NN) v_par[x] = 0; }
        match_wave_sync();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int x = lane + 64 * j;
            if (defect(x)) __hip_atomic_fetch_xor(s_par + v_label[x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        match_wave_sync();
        bool any = false;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int x = lane + 64 * j;
            if (x < n) { const u32 l = v_label[x]; any |= l != 0 && (v_par[l] & 1u); }
        }
        if (!__ballot(any) || r == round_bound) break;            // wave-uniform
        bool fresh = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u32 g0 = ed[k] >> UFP_G_SHIFT;
            if (g0 == 2) continue;
            const u32 la = v_label[ed[k] & 0xffu], lb = v_label[(ed[k] >> 8) & 0xffu];
            const u32 inc = (u32)(la != 0 && (v_par[la] & 1u)) + (u32)(lb != 0 && (v_par[lb] & 1u));
            const u32 g1 = min(2u, g0 + inc);
            ed[k] = (ed[k] & 0x00ffffffu) | g1 << UFP_G_SHIFT;
            fresh |= g1 == 2;
        }
        match_wave_sync();                                        // every lane has read the labels of this round before a union moves one
        if (!__ballot(fresh)) continue;                           // wave-uniform: no new full edge, the clusters stand
        for (int pass = 0; pass < NN; ++pass) {                   // (a label travels at least one edge per pass)
            bool changed = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (ed[k] >> UFP_G_SHIFT != 2) continue;
                const u32 a = ed[k] & 0xffu, b = (ed[k] >> 8) & 0xffu;
                const u32 la = v_label[a], lb = v_label[b];
                if (la != lb) {
                    __hip_atomic_fetch_min(s_label + (la < lb ? b : a), la < lb ? la : lb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    changed = true;
                }
            }
            match_wave_sync();
            if (!__ballot(changed)) break;                        // wave-uniform
        }
    }
    // ---- peeling: levels and parent edges ---------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int x = lane + 64 * j;
        if (x < NN) {
            s_level[x] = (u8)((x == B || v_label[x] == (u32)x + 1u) ? 0u : UFP_NOLEVEL);
            v_parent[x] = UFP_NONE;
            v_par[x] = defect(x);
        }
    }
    match_wave_sync();
    int deepest = 0;
    for (int lev = 1; lev < NN; ++lev) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (ed[k] >> UFP_G_SHIFT != 2) continue;
            const u32 a = ed[k] & 0xffu, b = (ed[k] >> 8) & 0xffu;
            const u32 va = s_level[a], vb = s_level[b];
            const u32 word = (u32)(lane + 64 * k) << 9 | ((ed[k] >> 16) & 1u) << 8;
            if (va == (u32)(lev - 1) && vb == UFP_NOLEVEL) __hip_atomic_fetch_min(s_parent + b, word | a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else if (vb == (u32)(lev - 1) && va == UFP_NOLEVEL) __hip_atomic_fetch_min(s_parent + a, word | b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        match_wave_sync();
        bool reached = false;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int x = lane + 64 * j;
            if (x < n && s_level[x] == UFP_NOLEVEL && v_parent[x] != UFP_NONE) { s_level[x] = (u8)lev; reached = true; }
        }
        match_wave_sync();
        if (!__ballot(reached)) break;                            // wave-uniform
        deepest = lev;
    }
    // ---- peeling: from the deepest level down ---------------------------------------------------------------------------------------------------------
    u32 cls = 0;
    for (int lev = deepest; lev >= 1; --lev) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int x = lane + 64 * j;
            if (x >= n || s_level[x] != (u32)lev || !(v_par[x] & 1u)) continue;
            const u32 word = v_parent[x];                         // (an edge is in the correction once: its lower end has one parent edge)
            __hip_atomic_fetch_xor(s_par + (word & 0xffu), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            cls ^= (word >> 8) & 1u;
        }
        match_wave_sync();
    }
    const int out = __popcll(__ballot(cls & 1u)) & 1;
    match_wave_sync();                                            // every lane is through with `s` before a following call reuses it
    return out;
}
