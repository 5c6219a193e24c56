// What the translation units around uf_wide_dev.h's component decode share (uf_wide.hip: streams; env_wide_uf.hip: the wide environment's volumes): the
// handle behind include/deepq_hip.h's dq_wide_uf and the register pinning of the values that live across a decode.
#pragma once
#include "uf_wide_dev.h"

#define UFW_NODE_SLOTS 128                                       // thread 128 c + j <-> node j of component c
// A uniform value that lives across the component decode is kept in a vector register: the decode needs the scalar ones, and four waves of at most 64 KiB of LDS
// have vector registers to spare (uf_stream.hip's STREAM_IN_VGPR).
#define UFW_IN_VGPR(x) asm volatile("" : "+v"(x))
#ifdef __HIPCC__
static __device__ __forceinline__ void ufw_layout_in_vgpr(UfwLayout& L) {
    UFW_IN_VGPR(L.o_frame); UFW_IN_VGPR(L.o_carry); UFW_IN_VGPR(L.o_acc); UFW_IN_VGPR(L.o_ring); UFW_IN_VGPR(L.o_label); UFW_IN_VGPR(L.o_par);
    UFW_IN_VGPR(L.o_parent); UFW_IN_VGPR(L.o_level); UFW_IN_VGPR(L.o_g); UFW_IN_VGPR(L.o_ex); UFW_IN_VGPR(L.o_ez); UFW_IN_VGPR(L.o_v);
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
