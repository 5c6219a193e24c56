// Device side of the union-find decoder, shared by uf_st.hip (uf_st_kernel: volumes given as cells, dq_decode_uf), the
// union-find forms of env_match.hip / env_guide.hip and uf_stream.hip (the sliding window of section 17): one Pauli component of one volume by one wavefront.
//
// Graph, unit weights, n nodes per round: node (u, t) = t n + u, the boundary node B = depth n (spatial and future boundary merged).  Edges of round t have
// ids t (d^2 + n) + k: k = q < d^2 the space edge of qubit q (its two plaquettes of the component in slice t, or its one plaquette and B), k = d^2 + u the
// time edge (u, t) -- (u, t + 1), in the last round (u, t) -- B.
// Growth in synchronous rounds: an edge carries g in {0, 1, 2}; a cluster is active when it holds an odd number of defects and not B; in a round every edge
// gains 1 per endpoint in an active cluster (capped at 2), then the ends of every full edge (g = 2) are united; until no cluster is active.  A cluster is
// the set of nodes with one label: the lowest of 0 for B and id + 1 for a node, spread over the full edges with LDS atomic minima until a pass changes
// nothing (the fixed point is the connected component's minimum, whatever the order).  So label 0 = "holds B", and label - 1 is the lowest node otherwise.
// Peeling over the full edges: roots (level 0) are B and the node label - 1 of every other cluster; levels by breadth-first search, the parent edge of a node =
// the lowest edge id joining it to the previous level (atomic minimum); from the deepest level down a node whose subtree holds an odd number of defects
// puts its parent edge into the correction and toggles its parent.
// Every loop bound is a constant of (d, depth), which the host validates (d <= 7, depth <= 16: at most 384 nodes + B and 1168 edges); every exit is
// wave-uniform and depends on the wave's own data.  All state is the wave's own LDS (UF_LDS bytes) and registers.
#pragma once
#include "match_dev.h"                                           // match_wave_sync

#define UF_MAX_DEPTH 16
#define UF_MAX_NODES 388                                         // 16 rounds of 24 nodes + B, padded
#define UF_MAX_EDGES 1168                                        // 16 (49 + 24)
#define UF_O_DW 0                                                // [2][16] defect words: bit u of word [comp][t] = defect (u, t)
#define UF_O_LABEL (UF_O_DW + 128)                               // u32 [nodes + 1] cluster label
#define UF_O_PAR (UF_O_LABEL + 4 * UF_MAX_NODES)                 // u32 [nodes + 1] defect parity per label; then subtree parity per node
#define UF_O_PARENT (UF_O_PAR + 4 * UF_MAX_NODES)                // u32 [nodes + 1] parent edge
#define UF_O_EA (UF_O_PARENT + 4 * UF_MAX_NODES)                 // u16 [edges] one end
#define UF_O_EB (UF_O_EA + 2 * UF_MAX_EDGES)                     // u16 [edges] the other
#define UF_O_LEVEL (UF_O_EB + 2 * UF_MAX_EDGES)                  // u16 [nodes + 1]
#define UF_O_G (UF_O_LEVEL + 2 * UF_MAX_NODES)                   // u8 [edges] growth
#define UF_LDS (UF_O_G + UF_MAX_EDGES)

struct UfComp {
    const u8* eu;           // [d^2] qubit -> its first plaquette of the component (node index)
    const u8* ev;           // [d^2] ... its second one, 255: none (the edge goes to B)
    int n, d2;
};

#define UF_NONE 0xffffffffu
#define UF_NOLEVEL 0xffffu

// One component of one volume: W = edges of the correction, M = XOR of the qubits of its space edges, rounds = growth rounds made; wave-uniform.
// Commit (the sliding window of uf_stream.hip): unless `final`, only the edges of rounds t < commit count into W and M, and
// carry = the set of u (bit u) whose time edge of round commit - 1 is in the correction.  Without Commit the two arguments are not read.
// Closed (a stream that ends on a round of perfect measurements): in a `final` window the time edges of the last round do not exist.
// They are the last n edge ids, and the growth loop stops in front of them: never grown, they are never full, so no label crosses them, no level reaches
// across them and they are never in the correction.
template <bool Commit, bool Closed = false>
static __device__ __forceinline__ void uf_component_impl(const UfComp& G, int depth, volatile u32* dw, u8* __restrict__ s, int lane, int commit, bool final, int& Wout,
                                                         u64& Mout, u32& carry_out, int& ndef, int& rounds_out) {
    u32* s_label = reinterpret_cast<u32*>(s + UF_O_LABEL);
    u32* s_par = reinterpret_cast<u32*>(s + UF_O_PAR);
    u32* s_parent = reinterpret_cast<u32*>(s + UF_O_PARENT);
    volatile u32* v_label = s_label;
    volatile u32* v_par = s_par;
    volatile u32* v_parent = s_parent;
    volatile uint16_t* s_ea = reinterpret_cast<volatile uint16_t*>(s + UF_O_EA);
    volatile uint16_t* s_eb = reinterpret_cast<volatile uint16_t*>(s + UF_O_EB);
    volatile uint16_t* s_level = reinterpret_cast<volatile uint16_t*>(s + UF_O_LEVEL);
    volatile u8* s_g = s + UF_O_G;
    const int n = G.n, d2 = G.d2, per_round = d2 + n;
    const int B = depth * n, NN = B + 1, NE = depth * per_round;
    const int NE_grown = Closed && final ? NE - n : NE;
    int total = 0;
    for (int t = 0; t < depth; ++t) total += __popc(dw[t]);       // wave-uniform
    ndef = total;
    Wout = 0; Mout = 0; rounds_out = 0;
    if (Commit) carry_out = 0;
    if (total == 0) return;                                       // wave-uniform: nothing to correct, `s` untouched
    auto defect = [&](int x) -> u32 { const int t = x / n; return x < B ? (dw[t] >> (x - t * n)) & 1u : 0u; };
    // ---- edges and singleton clusters --------------------------------------------------------------------------------------------------------
    for (int e = lane; e < NE; e += 64) {
        const int t = e / per_round, k = e - t * per_round;
        int a, b;
        if (k < d2) {
            const int u = G.eu[k], v = G.ev[k];
            a = u == 255 ? B : t * n + u;
            b = (u == 255 || v == 255) ? B : t * n + v;
        } else {
            a = t * n + (k - d2);
            b = t + 1 < depth ? a + n : B;
        }
        s_ea[e] = (uint16_t)a; s_eb[e] = (uint16_t)b; s_g[e] = 0;
    }
    for (int x = lane; x < NN; x += 64) v_label[x] = x == B ? 0u : (u32)x + 1u;
    match_wave_sync();
    // ---- growth ---------------------------------------------------------------------------------------------------------------------------------
    int rounds = 0;
    const int round_bound = 2 * NE;
    for (int r = 0; r <= round_bound; ++r) {
        for (int x = lane; x < NN; x += 64) v_par[x] = 0;
        match_wave_sync();
        for (int x = lane; x < B; x += 64)
            if (defect(x)) __hip_atomic_fetch_xor(s_par + v_label[x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        match_wave_sync();
        bool any = false;
        for (int x = lane; x < B; x += 64) { const u32 l = v_label[x]; any |= l != 0 && (v_par[l] & 1u); }
        if (!__ballot(any) || r == round_bound) break;            // wave-uniform
        ++rounds;
        bool fresh = false;
        for (int e = lane; e < NE_grown; e += 64) {
            const u32 la = v_label[s_ea[e]], lb = v_label[s_eb[e]];
            const int inc = (int)(la != 0 && (v_par[la] & 1u)) + (int)(lb != 0 && (v_par[lb] & 1u));
            const int g0 = s_g[e], g1 = min(2, g0 + inc);
            if (g1 != g0) { s_g[e] = (u8)g1; fresh |= g1 == 2; }
        }
        match_wave_sync();
        if (!__ballot(fresh)) continue;                           // wave-uniform: no new full edge, the clusters stand
        for (int pass = 0; pass < NN; ++pass) {                   // (a label travels at least one edge per pass)
            bool changed = false;
            for (int e = lane; e < NE; e += 64) {
                if (s_g[e] != 2) continue;
                const int a = s_ea[e], b = s_eb[e];
                const u32 la = v_label[a], lb = v_label[b];
                if (la != lb) {
                    const u32 m = la < lb ? la : lb;
                    __hip_atomic_fetch_min(s_label + (la < lb ? b : a), m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    changed = true;
                }
            }
            match_wave_sync();
            if (!__ballot(changed)) break;                        // wave-uniform
        }
    }
    // ---- peeling: levels and parent edges ---------------------------------------------------------------------------------------------------------
    for (int x = lane; x < NN; x += 64) {
        s_level[x] = (uint16_t)((x == B || v_label[x] == (u32)x + 1u) ? 0u : UF_NOLEVEL);
        v_parent[x] = UF_NONE;
        v_par[x] = defect(x);
    }
    match_wave_sync();
    int deepest = 0;
    for (int lev = 1; lev < NN; ++lev) {
        for (int e = lane; e < NE; e += 64) {
            if (s_g[e] != 2) continue;
            const int a = s_ea[e], b = s_eb[e];
            const u32 va = s_level[a], vb = s_level[b];
            if (va == (u32)(lev - 1) && vb == UF_NOLEVEL) __hip_atomic_fetch_min(s_parent + b, (u32)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else if (vb == (u32)(lev - 1) && va == UF_NOLEVEL) __hip_atomic_fetch_min(s_parent + a, (u32)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        match_wave_sync();
        bool reached = false;
        for (int x = lane; x < B; x += 64)
            if (s_level[x] == UF_NOLEVEL && v_parent[x] != UF_NONE) { s_level[x] = (uint16_t)lev; reached = true; }
        match_wave_sync();
        if (!__ballot(reached)) break;                            // wave-uniform
        deepest = lev;
    }
    // ---- peeling: from the deepest level down ---------------------------------------------------------------------------------------------------------
    int w = 0;
    u64 m = 0;
    u32 cr = 0;
    for (int lev = deepest; lev >= 1; --lev) {
        for (int x = lane; x < B; x += 64) {
            if (s_level[x] != (u32)lev || !(v_par[x] & 1u)) continue;
            const int e = (int)v_parent[x];
            const int a = s_ea[e], up = a == x ? (int)s_eb[e] : a;
            __hip_atomic_fetch_xor(s_par + up, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const int k = e % per_round;
            if (Commit && !final) {                               // (an edge is in the correction once: its lower end has one parent edge)
                const int t = e / per_round;
                if (t >= commit) continue;
                if (k >= d2 && t == commit - 1) cr |= 1u << (k - d2);
            }
            ++w;
            if (k < d2) m ^= 1ull << k;
        }
        match_wave_sync();
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) { w += __shfl_xor(w, k); m ^= (u64)__shfl_xor((unsigned long long)m, k); }
    if (Commit) {
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) cr |= (u32)__shfl_xor((int)cr, k);
        carry_out = __builtin_amdgcn_readfirstlane(cr);
    }
    match_wave_sync();                                            // every lane is through with `s` before the next component reuses it
    Wout = __builtin_amdgcn_readfirstlane(w);
    const u32 lo = __builtin_amdgcn_readfirstlane((u32)m), hi = __builtin_amdgcn_readfirstlane((u32)(m >> 32));
    Mout = (u64)lo | (u64)hi << 32;
    rounds_out = rounds;
}

static __device__ __forceinline__ void uf_component(const UfComp& G, int depth, volatile u32* dw, u8* __restrict__ s, int lane, int& Wout, u64& Mout, int& ndef,
                                                    int& rounds_out) {
    u32 carry;
    uf_component_impl<false>(G, depth, dw, s, lane, depth, true, Wout, Mout, carry, ndef, rounds_out);
}

// One component of one window of a stream: uf_component on the depth-`depth` graph, of whose correction the rounds t < commit are committed (all of it when
// `final`: W and M are then uf_component's); carry: a wave-uniform word, bit u = the time edge (u, commit - 1) is in the correction.  ndef counts the window's
// defect rows as they stand in `dw`.  Closed: see uf_component_impl.
template <bool Closed = false>
static __device__ __forceinline__ void uf_component_commit(const UfComp& G, int depth, volatile u32* dw, u8* __restrict__ s, int lane, int commit, bool final, int& Wout,
                                                           u64& Mout, u32& carry, int& ndef, int& rounds_out) {
    uf_component_impl<true, Closed>(G, depth, dw, s, lane, commit, final, Wout, Mout, carry, ndef, rounds_out);
}
