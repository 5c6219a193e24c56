// Device side of the space-time matching decoder (DESIGN.md sections 13 and 14), shared by match_st.hip (match_st_kernel: volumes given as cells,
// dq_decode_match) and env_match.hip (env_match_kernel: the current volume of a lattice of the environment, dq_env_match_select): the handle's tables
// and the matching of one Pauli component of one volume by one wavefront.  The graph, the open future boundary, the tie rules and the 14 / 32
// fallback are stated at the top of match_st.hip.
#pragma once
#include "match_dev.h"
#include "uf_dev.h"

#define MST_O_T DQ_MATCH_LDS                    // [32] round of defect i (its node sits in match_dev.h's list bytes)
#define MST_O_DW (MST_O_T + 32)                 // [2][16] defect words: bit u of word [comp][t] = defect (u, t)
#define MST_LDS (MST_O_DW + 128)
#define MST_MAX_DEPTH 16

struct MatchStComp {
    const u8* dist;         // [n][n][2]  lattice_match_tables
    const u8* distB;        // [n][2]
    const u64* path;        // [n][n][2]  lattice_match_paths: qubit masks of one shortest path per entry
    const u64* pathB;       // [n][2]
    int n;
};

struct MatchStTables {
    u8* blob;               // one device allocation behind all the pointers
    MatchStComp comp[2];
    const u8* cell;         // [64] lane 32 c + j -> grid cell a (d + 1) + b of node j of component c (255: none)
    const u8* stab;         // [64] lane 32 c + j -> bit of node j of component c in a syndrome word of the environment (measurement order; 255: none)
    UfComp uf[2];           // uf_dev.h: the union-find decoder's endpoint tables, qubit -> (u, v or none), [2][64] bytes per component
};

static __device__ __forceinline__ u64 mst_bcast(u64 x) {
    const u32 lo = __builtin_amdgcn_readfirstlane((u32)x), hi = __builtin_amdgcn_readfirstlane((u32)(x >> 32));
    return (u64)lo | (u64)hi << 32;
}

// One component of one volume: W = the matching's weight, M = the XOR of its paths' qubit masks; wave-uniform.
static __device__ __forceinline__ void mst_component(const MatchStComp& T, int depth, volatile u32* dw, u8* __restrict__ s, int lane, int& Wout, u64& Mout,
                                                     int& ndef, int* inexact) {
    volatile u8* s_node = s;                                      // [32] node of defect i
    volatile u8* s_pb = s + DQ_MATCH_O_PB;                        // [32][2] boundary distances (class 0: spatial or future)
    volatile u32* s_adj = reinterpret_cast<volatile u32*>(s + DQ_MATCH_O_ADJ);
    volatile u8* s_comp = s + DQ_MATCH_O_COMP;
    volatile u8* s_cl = s + DQ_MATCH_O_CL;
    volatile u8* s_pd = s + DQ_MATCH_O_PD;                        // [32][32][2]
    volatile u8* f = s + DQ_MATCH_O_F;
    volatile u8* s_t = s + MST_O_T;                               // [32] round of defect i
    const int BIG = DQ_MATCH_BIGW;
    const int n = T.n;
    // the nearest boundary of a defect that is not solved exactly
    auto to_boundary = [&](int node, int t, int& add, int& par, u64& m) {
        const int b0s = T.distB[2 * node], b1 = T.distB[2 * node + 1], fb = depth - t;
        const int b0 = min(b0s, fb);
        const int cp = b1 < b0;
        add += cp ? b1 : b0;
        par ^= cp;
        m ^= cp ? T.pathB[2 * node + 1] : (fb < b0s ? 0ull : T.pathB[2 * node]);
    };
    auto wave_reduce = [&](int& add, int& par, u64& m) {
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) { add += __shfl_xor(add, k); par ^= __shfl_xor(par, k); m ^= (u64)__shfl_xor((unsigned long long)m, k); }
    };
    // ---- defect list in (t, node) order --------------------------------------------------------------------------------------------------
    int total = 0, extra_add = 0, extra_par = 0;
    u64 extra_m = 0;
    for (int t = 0; t < depth; ++t) {
        const u32 D = dw[t];                                      // wave-uniform
        if (lane < n && ((D >> lane) & 1)) {
            const int rank = total + __popc(D & ((1u << lane) - 1u));
            if (rank < DQ_MATCH_MAX_LIST) { s_node[rank] = (u8)lane; s_t[rank] = (u8)t; }
            else to_boundary(lane, t, extra_add, extra_par, extra_m);
        }
        total += __popc(D);
    }
    ndef = total;
    const int L = total < DQ_MATCH_MAX_LIST ? total : DQ_MATCH_MAX_LIST;
    if (total > L) {                                              // wave-uniform
        wave_reduce(extra_add, extra_par, extra_m);
        *inexact |= 1;
    }
    match_wave_sync();
    // ---- distances among the L defects ----------------------------------------------------------------------------------------------------
    for (int x = lane; x < L * L; x += 64) {
        const int i = x / L, j = x - i * L;
        const u8* p = T.dist + ((size_t)s_node[i] * n + s_node[j]) * 2;
        const int ti = s_t[i], tj = s_t[j], dt = ti < tj ? tj - ti : ti - tj;
        const int p0 = p[0], p1 = p[1];
        s_pd[(i * 32 + j) * 2] = (u8)(p0 == 255 ? 255 : min(p0 + dt, 254));
        s_pd[(i * 32 + j) * 2 + 1] = (u8)(p1 == 255 ? 255 : min(p1 + dt, 254));
    }
    if (lane < L) {
        const int node = s_node[lane], fb = depth - (int)s_t[lane];
        s_pb[2 * lane] = (u8)min((int)T.distB[2 * node], fb);
        s_pb[2 * lane + 1] = T.distB[2 * node + 1];
    }
    match_wave_sync();
    // ---- clusters (match_dev.h match_classify's rule and label propagation) ------------------------------------------------------------------
    int comp = lane;
    if (lane < L) {
        u32 adj = 0;
        const int bi0 = s_pb[2 * lane] == 255 ? BIG : s_pb[2 * lane], bi1 = s_pb[2 * lane + 1] == 255 ? BIG : s_pb[2 * lane + 1];
        for (int j = 0; j < L; ++j) {
            if (j == lane) continue;
            const int bj0 = s_pb[2 * j] == 255 ? BIG : s_pb[2 * j], bj1 = s_pb[2 * j + 1] == 255 ? BIG : s_pb[2 * j + 1];
            const int p0 = s_pd[(lane * 32 + j) * 2], p1 = s_pd[(lane * 32 + j) * 2 + 1];
            const bool c0 = p0 != 255 && p0 < min(bi0 + bj0, bi1 + bj1);
            const bool c1 = p1 != 255 && p1 < min(bi0 + bj1, bi1 + bj0);
            if (c0 || c1) adj |= 1u << j;
        }
        s_adj[lane] = adj;
        s_comp[lane] = (u8)lane;
    }
    match_wave_sync();
    for (int it = 0; it < DQ_MATCH_MAX_LIST; ++it) {
        int nc = comp;
        if (lane < L)
            for (u32 m = s_adj[lane]; m; m &= m - 1) nc = min(nc, (int)s_comp[__builtin_ctz(m)]);
        const bool changed = lane < L && nc != comp;
        match_wave_sync();
        if (changed) { comp = nc; s_comp[lane] = (u8)nc; }
        match_wave_sync();
        if (!__ballot(changed)) break;                            // wave-uniform
    }
    // ---- the clusters in the order of their lowest defect: DP, walk back, combine ------------------------------------------------------------
    auto LD = [&](int idx) -> int { const int v = f[idx]; return v == 255 ? BIG : v; };
    int W0 = 0, W1 = BIG;
    u64 M0 = 0, M1 = 0;
    u64 reps = __ballot(lane < L && comp == lane);
    while (reps) {                                                // wave-uniform; at most DQ_MATCH_MAX_LIST clusters
        const int rep = __builtin_ctzll(reps);
        reps &= reps - 1;
        const u64 members = __ballot(lane < L && comp == rep);
        const int msize = __popcll(members);
        const int k = msize < DQ_MATCH_MAX_DEFECTS ? msize : DQ_MATCH_MAX_DEFECTS;
        int cl_add = 0, cl_par = 0;
        u64 cl_m = 0;
        if ((members >> lane) & 1) {
            const int rank = __popcll(members & ((1ull << lane) - 1));
            if (rank < k) s_cl[rank] = (u8)lane;
            else to_boundary(s_node[lane], s_t[lane], cl_add, cl_par, cl_m);
        }
        match_wave_sync();
        int w0, w1;
        match_dp_lds(s_cl, s_pd, s_pb, f, k, lane, w0, w1);
        // one lane walks the table back from the full set, for either class: at each step the set's highest member goes to the boundary or to a partner,
        // the first candidate (boundary class 0, class 1, partners ascending) that reproduces the entry
        u64 cm0 = 0, cm1 = 0;
        if (lane == 0) {
            for (int c0 = 0; c0 < 2; ++c0) {
                if ((c0 ? w1 : w0) >= BIG) continue;
                int S = (1 << k) - 1, c = c0;
                u64 m = 0;
                for (int step = 0; step < DQ_MATCH_MAX_DEFECTS && S; ++step) {
                    const int h = 31 - __clz(S), r = S ^ (1 << h), ch = s_cl[h];
                    const int target = LD(2 * S + c);
                    const int b0 = s_pb[2 * ch] == 255 ? BIG : s_pb[2 * ch], b1 = s_pb[2 * ch + 1] == 255 ? BIG : s_pb[2 * ch + 1];
                    const int node = s_node[ch], t = s_t[ch];
                    int nS = -1, nc = c;
                    u64 pm = 0;
                    if (LD(2 * r + c) + b0 == target) {
                        nS = r;
                        pm = depth - t < (int)T.distB[2 * node] ? 0ull : T.pathB[2 * node];
                    } else if (LD(2 * r + (c ^ 1)) + b1 == target) {
                        nS = r; nc = c ^ 1;
                        pm = T.pathB[2 * node + 1];
                    } else {
                        for (int mm = r; mm && nS < 0; mm &= mm - 1) {
                            const int v = __builtin_ctz(mm), rr = r ^ (1 << v), cv = s_cl[v];
                            const int d0 = s_pd[(ch * 32 + cv) * 2] == 255 ? BIG : s_pd[(ch * 32 + cv) * 2];
                            const int d1 = s_pd[(ch * 32 + cv) * 2 + 1] == 255 ? BIG : s_pd[(ch * 32 + cv) * 2 + 1];
                            const u64* pp = T.path + ((size_t)node * n + s_node[cv]) * 2;
                            if (LD(2 * rr + c) + d0 == target) { nS = rr; pm = pp[0]; }
                            else if (LD(2 * rr + (c ^ 1)) + d1 == target) { nS = rr; nc = c ^ 1; pm = pp[1]; }
                        }
                    }
                    if (nS < 0) break;                            // (every reachable entry has a candidate that reproduces it)
                    m ^= pm; S = nS; c = nc;
                }
                if (c0) cm1 = m; else cm0 = m;
            }
        }
        u64 m0 = mst_bcast(cm0), m1 = mst_bcast(cm1);
        match_wave_sync();                                        // the walk is through with the table before the next cluster's lists are written
        if (msize > k) {                                          // wave-uniform
            wave_reduce(cl_add, cl_par, cl_m);
            if (cl_par) { const int tw = w0; w0 = w1; w1 = tw; const u64 tm = m0; m0 = m1; m1 = tm; }
            w0 = min(w0 + cl_add, BIG); w1 = min(w1 + cl_add, BIG);
            m0 ^= cl_m; m1 ^= cl_m;
            *inexact |= 1;
        }
        const int a00 = W0 + w0, a11 = W1 + w1, a01 = W0 + w1, a10 = W1 + w0;
        const u64 n0m = a00 <= a11 ? M0 ^ m0 : M1 ^ m1, n1m = a01 <= a10 ? M0 ^ m1 : M1 ^ m0;
        W0 = min(min(a00, a11), BIG); W1 = min(min(a01, a10), BIG);
        M0 = n0m; M1 = n1m;
    }
    if (extra_par) { const int tw = W0; W0 = W1; W1 = tw; const u64 tm = M0; M0 = M1; M1 = tm; }
    W0 += extra_add; W1 += extra_add;
    M0 ^= extra_m; M1 ^= extra_m;
    match_wave_sync();                                            // every lane is through with `s` before the next component reuses it
    const bool one = W1 < W0;
    Wout = __builtin_amdgcn_readfirstlane(one ? W1 : W0);
    Mout = mst_bcast(one ? M1 : M0);
}
