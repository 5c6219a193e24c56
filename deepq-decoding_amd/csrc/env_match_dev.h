// The matching decoder's next action for ONE lattice of the environment by one wavefront, shared by env_match.hip (env_match_kernel: every lattice,
// dq_env_match_select) and env_guide.hip (env_guided_select_kernel: the lattices whose policy draw follows the teacher, dq_env_guided_select).  The rule is
// stated at the top of env_match.hip; DESIGN.md sections 14 and 15.
#pragma once
#include "match_st_dev.h"
#include "env_dev.h"
#include "decode_eval.h"

// The component solver of env_match_wave, a compile-time choice: the matching (match_st_dev.h mst_component, MST_LDS bytes per wave) or the union-find
// decoder (uf_dev.h uf_component, UF_LDS bytes; no fallback, so its flag stays 0).
struct EnvSolveMatching {
    typedef MatchStComp Comp;
    static constexpr int O_DW = MST_O_DW, DW_STRIDE = MST_MAX_DEPTH;
    static __device__ __forceinline__ void solve(const Comp& T, int depth, volatile u32* dw, u8* s, int lane, int& W, u64& M, int& nd, int& flag) {
        mst_component(T, depth, dw, s, lane, W, M, nd, &flag);
    }
};
struct EnvSolveUnionFind {
    typedef UfComp Comp;
    static constexpr int O_DW = UF_O_DW, DW_STRIDE = UF_MAX_DEPTH;
    static __device__ __forceinline__ void solve(const Comp& T, int depth, volatile u32* dw, u8* s, int lane, int& W, u64& M, int& nd, int& flag) {
        int rounds;
        uf_component(T, depth, dw, s, lane, W, M, nd, rounds);
    }
};

// `word`: lane < sw holds word `lane` of the lattice's record (STATE_FIXED words, then the current volume's syndrome words); smem: the solver's LDS bytes owned by the
// wave.  Returns the action (wave-uniform), flag = the matching's 14 / 32 fallback flag of the volume (0 for a lattice whose done flag is set: it gets the
// identity, the step resets it whatever the action).
template <class Solver>
static __device__ __forceinline__ int env_match_wave(const typename Solver::Comp& c0, const typename Solver::Comp& c1, const u8* __restrict__ stab, u64 word, int d2, int depth,
                                                     int model, int use_Y, int identity, u8* smem, int lane, int& flag) {
    flag = 0;
    const u64 done0 = wave_bcast64(word, 4), done1 = wave_bcast64(word, 5);     // completed_actions
    if ((wave_bcast64(word, 8) >> 32) & 1) return identity;                     // done (wave-uniform)
    volatile u32* s_dw = reinterpret_cast<volatile u32*>(smem + Solver::O_DW);
    // lanes 0 .. n - 1 pick component 0's nodes out of the round's syndrome word, lanes 32 .. 32 + n - 1 component 1's: a ballot is the round's two words
    const int my_bit = stab[lane];
    u64 prev = 0;
    for (int t = 0; t < depth; ++t) {
        const u64 sword = wave_bcast64(word, STATE_FIXED + t);
        const u64 cur = __ballot(my_bit < 64 && ((sword >> (my_bit & 63)) & 1));
        const u64 D = cur ^ prev;
        prev = cur;
        if (lane == 0) { s_dw[t] = (u32)D; s_dw[Solver::DW_STRIDE + t] = (u32)(D >> 32); }
    }
    match_wave_sync();
    int w[2], nd[2];
    u64 m[2];
    Solver::solve(c0, depth, s_dw, smem, lane, w[0], m[0], nd[0], flag);
    Solver::solve(c1, depth, s_dw + Solver::DW_STRIDE, smem, lane, w[1], m[1], nd[1], flag);
    // the frame as action indices (decode.hip's layer-to-Pauli map: X model 1; use_Y: layer + 1; else layer 0 -> X, layer 1 -> Z)
    const u64 qubits = d2 < 64 ? (1ull << d2) - 1 : ~0ull;
    const u64 fx = m[0] & qubits, fz = model == DQ_MODEL_X ? 0ull : m[1] & qubits;      // (X model: no action layer for component 1)
    u64 want0 = 0, want1 = 0;
    if (model == DQ_MODEL_X) {
        want0 = fx;
    } else if (use_Y) {
        or_shl128(want0, want1, fx & ~fz, 0);
        or_shl128(want0, want1, fx & fz, d2);
        or_shl128(want0, want1, fz & ~fx, 2 * d2);
    } else {
        or_shl128(want0, want1, fx, 0);
        or_shl128(want0, want1, fz, d2);
    }
    want0 &= ~done0; want1 &= ~done1;
    return want0 ? __builtin_ctzll(want0) : (want1 ? 64 + __builtin_ctzll(want1) : identity);
}

// env_match.hip: what dq_env_match_select and dq_env_guided_select check alike -- `ev` is of the environment's lattice (DQ_ERR_INVALID), the lattice is
// covered (DQ_ERR_UNSUPPORTED) -- and the handle's matching tables, built at its first call.  `who`: the entry point's name for the message.
dq_status env_match_prepare(const dq_env* env, dq_decode_eval* V, EnvStateView* S, const char* who);
