// The union-find decoder on faulty syndrome volumes (include/deepq_hip.h dq_decode_uf): the second baseline beside the space-time
// matching of match_st.hip, on the same defects D_t = S_t xor S_{t-1} (S_-1 = 0), the same unit-weight graph with the open future boundary, both Pauli
// components independently.  One wavefront per volume, one wave per block: match_st_kernel's ballot front end and frame store around uf_dev.h's uf_component.
// The algorithm -- synchronous cluster growth, then peeling of a breadth-first forest -- is stated at the top of uf_dev.h; it has no cluster-size limit
// and so no fallback.  Everything a volume needs lives in its wave's LDS (UF_LDS bytes) and registers: no scratch pool, no lock, no loop whose exit depends on
// another wave; every loop bound follows from (d, depth), which the entry point validates.
#include "uf_dev.h"
#include "match_st_dev.h"
#include "decode_eval.h"

namespace {

__global__ __launch_bounds__(64) void uf_st_kernel(UfComp c0, UfComp c1, const u8* __restrict__ cell, const u8* __restrict__ volumes, int nvol, int d, int depth,
                                                   u8* __restrict__ frame, int32_t* __restrict__ weight, int32_t* __restrict__ n_defects,
                                                   int32_t* __restrict__ rounds) {
    __shared__ __attribute__((aligned(16))) u8 smem[UF_LDS];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= nvol) return;
    const int G = (d + 1) * (d + 1), d2 = d * d;
    volatile u32* s_dw = reinterpret_cast<volatile u32*>(smem + UF_O_DW);
    // lanes 0 .. n - 1 read component 0's nodes, lanes 32 .. 32 + n - 1 component 1's: a ballot is the round's two syndrome words
    const int my_cell = cell[lane];
    const u8* vp = volumes + (size_t)i * depth * G;
    u64 prev = 0;
    for (int t = 0; t < depth; ++t) {
        const u64 cur = __ballot(my_cell < G && vp[t * G + (my_cell < G ? my_cell : 0)] != 0);
        const u64 D = cur ^ prev;
        prev = cur;
        if (lane == 0) { s_dw[t] = (u32)D; s_dw[UF_MAX_DEPTH + t] = (u32)(D >> 32); }
    }
    match_wave_sync();
    int w[2], nd[2], rd[2];
    u64 m[2];
    uf_component(c0, depth, s_dw, smem, lane, w[0], m[0], nd[0], rd[0]);
    uf_component(c1, depth, s_dw + UF_MAX_DEPTH, smem, lane, w[1], m[1], nd[1], rd[1]);
    if (lane < d2) {                                              // hidden_state codes: component 0 = X (1), component 1 = Z (3), both = Y (2)
        const int x = (int)((m[0] >> lane) & 1), z = (int)((m[1] >> lane) & 1);
        frame[(size_t)i * d2 + lane] = (u8)(x ? (z ? 2 : 1) : (z ? 3 : 0));
    }
    if (lane < 2) {
        if (weight) weight[2 * (size_t)i + lane] = lane ? w[1] : w[0];
        if (n_defects) n_defects[2 * (size_t)i + lane] = lane ? nd[1] : nd[0];
        if (rounds) rounds[2 * (size_t)i + lane] = lane ? rd[1] : rd[0];
    }
}

}  // namespace

extern "C" {

dq_status dq_decode_uf(dq_decode_eval* V, const uint8_t* volumes_dev, int n, uint8_t* frame_dev, int32_t* weight_dev, int32_t* n_defects_dev, int32_t* rounds_dev,
                       void* stream) {
    DQ_REQUIRE(V && volumes_dev && frame_dev, DQ_ERR_INVALID, "dq_decode_uf: null argument");
    DQ_REQUIRE(n >= 1 && n <= V->max_volumes, DQ_ERR_INVALID, "dq_decode_uf: n = %d outside 1..max_volumes %d", n, V->max_volumes);
    DQ_REQUIRE(((reinterpret_cast<uintptr_t>(weight_dev) | reinterpret_cast<uintptr_t>(n_defects_dev) | reinterpret_cast<uintptr_t>(rounds_dev)) & 3) == 0,
               DQ_ERR_INVALID, "dq_decode_uf: weight_dev, n_defects_dev and rounds_dev must be 4-byte aligned");
    DQ_REQUIRE(V->d <= 7 && V->depth >= 1 && V->depth <= UF_MAX_DEPTH, DQ_ERR_UNSUPPORTED, "dq_decode_uf: d = %d, volume_depth = %d: union-find covers d <= 7, depth <= %d",
               V->d, V->depth, UF_MAX_DEPTH);
    const dq_status rc = match_st_tables(V);
    if (rc != DQ_OK) return rc;
    const MatchStTables* T = V->match_st;
    uf_st_kernel<<<n, 64, 0, (hipStream_t)stream>>>(T->uf[0], T->uf[1], T->cell, volumes_dev, n, V->d, V->depth, frame_dev, weight_dev, n_defects_dev, rounds_dev);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

}  // extern "C"
