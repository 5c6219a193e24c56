// Space-time minimum-weight matching of faulty syndrome volumes (include/deepq_hip.h dq_decode_match): the baseline a trained
// agent's failure rate is quoted against.  Per Pauli component the defects D_t = S_t xor S_{t-1} (S_-1 = 0) of the volume's rounds are nodes (u, t) of
// the component's graph (match_dev.h / lattice_host.h) times the time axis, unit weights everywhere:
//   (u, t1) -> (v, t2) with class c:  dist[u][v][c] + |t1 - t2|         (data errors in space, measurement errors in time)
//   (u, t)  -> the spatial boundary with class c:  distB[u][c]
//   (u, t)  -> the FUTURE boundary with class 0:   depth - t             (the volume ends on a faulty round: a measurement error of the last round is one-ended)
// One wavefront per volume: syndrome words by ballot, the defect list as (node, t) pairs, match_dev.h's cluster rule with min(distB[u][0], depth - t)
// as the class-0 boundary option (the rule's argument holds for any set of boundary paths), match_dp_lds per cluster, then one lane walks the
// table back from the full set for either class and XORs the chosen paths' qubit masks (lattice_match_paths); the clusters' (weight, mask) pairs
// combine by the (min, +) XOR-convolution.  The matching is the lightest over both classes (no w10 term: a decoder, not the referee's strict-class rule).
// Everything a volume needs lives in its wave's LDS and registers: no scratch pool, no lock, no loop whose exit depends on another wave.
// Fallback, flagged inexact: defects beyond the first DQ_MATCH_MAX_LIST of a component (in (t, node) order) and members of a cluster beyond its
// first DQ_MATCH_MAX_DEFECTS go to their nearest boundary (ties: class 0, then the spatial one).
#include "match_st_dev.h"
#include "lattice_host.h"
#include "decode_eval.h"

namespace {

__global__ __launch_bounds__(64) void match_st_kernel(MatchStComp c0, MatchStComp c1, const u8* __restrict__ cell, const u8* __restrict__ volumes, int nvol, int d,
                                                      int depth, u8* __restrict__ frame, int32_t* __restrict__ weight, int32_t* __restrict__ n_defects,
                                                      u8* __restrict__ inexact) {
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= nvol) return;
    const int G = (d + 1) * (d + 1), d2 = d * d;
    volatile u32* s_dw = reinterpret_cast<volatile u32*>(smem + MST_O_DW);
    // lanes 0 .. n - 1 read component 0's nodes, lanes 32 .. 32 + n - 1 component 1's: a ballot is the round's two syndrome words
    const int my_cell = cell[lane];
    const u8* vp = volumes + (size_t)i * depth * G;
    u64 prev = 0;
    for (int t = 0; t < depth; ++t) {
        const u64 cur = __ballot(my_cell < G && vp[t * G + (my_cell < G ? my_cell : 0)] != 0);
        const u64 D = cur ^ prev;
        prev = cur;
        if (lane == 0) { s_dw[t] = (u32)D; s_dw[MST_MAX_DEPTH + t] = (u32)(D >> 32); }
    }
    match_wave_sync();
    int flag = 0, w[2], nd[2];
    u64 m[2];
    mst_component(c0, depth, s_dw, smem, lane, w[0], m[0], nd[0], &flag);
    mst_component(c1, depth, s_dw + MST_MAX_DEPTH, smem, lane, w[1], m[1], nd[1], &flag);
    if (lane < d2) {                                              // hidden_state codes: component 0 = X (1), component 1 = Z (3), both = Y (2)
        const int x = (int)((m[0] >> lane) & 1), z = (int)((m[1] >> lane) & 1);
        frame[(size_t)i * d2 + lane] = (u8)(x ? (z ? 2 : 1) : (z ? 3 : 0));
    }
    if (lane < 2) {
        if (weight) weight[2 * (size_t)i + lane] = lane ? w[1] : w[0];
        if (n_defects) n_defects[2 * (size_t)i + lane] = lane ? nd[1] : nd[0];
    }
    if (lane == 0 && inexact) inexact[i] = (u8)flag;
}

}  // namespace

void match_st_free(MatchStTables* t) {
    if (!t) return;
    if (t->blob) (void)hipFree(t->blob);
    delete t;
}

// The handle's tables: built on the host and uploaded in one piece at the first dq_decode_match / dq_decode_uf / dq_env_*_select of the handle.
dq_status match_st_tables(dq_decode_eval* V) {
    if (V->match_st) return DQ_OK;
    LatticeHost L;
    lattice_build(V->d, &L);
    std::vector<u8> dist[2], distB[2], cell(64, 255), stab(64, 255), ends(256, 255);      // ends: [comp][eu, ev][64] (uf_dev.h UfComp)
    std::vector<u64> path[2], pathB[2];
    size_t off64[2][2], off8[2][2], bytes = 0;
    for (int c = 0; c < 2; ++c) {
        int w10;
        lattice_match_tables(L, c, &dist[c], &distB[c], &w10);
        lattice_match_paths(L, c, &path[c], &pathB[c]);
        const int n = (int)L.typed[c].size();
        DQ_REQUIRE(n <= 32 && V->d * V->d <= 64, DQ_ERR_UNSUPPORTED, "dq_decode_match: d = %d: a component's %d nodes do not fit half a wavefront", V->d, n);
        for (int j = 0; j < n; ++j) { const int s = L.typed[c][j]; cell[32 * c + j] = (u8)(L.sa[s] * (V->d + 1) + L.sb[s]); stab[32 * c + j] = (u8)s; }
        const int typ = c == 0 ? 3 : 1;
        for (int q = 0; q < V->d * V->d; ++q) {                           // the qubit's plaquettes of the component, as lattice_match_tables walks them
            int ne = 0;
            for (int s : L.qubit_stabs[q]) if (L.stab_type[s] == typ && ne < 2) ends[128 * c + 64 * ne++ + q] = (u8)L.ref_bit[s];
        }
        off64[c][0] = bytes; bytes += path[c].size() * sizeof(u64);
        off64[c][1] = bytes; bytes += pathB[c].size() * sizeof(u64);
    }
    for (int c = 0; c < 2; ++c) {
        off8[c][0] = bytes; bytes += dist[c].size();
        off8[c][1] = bytes; bytes += distB[c].size();
    }
    const size_t off_cell = bytes;
    bytes += cell.size();
    const size_t off_stab = bytes;
    bytes += stab.size();
    const size_t off_ends = bytes;
    bytes += ends.size();
    std::vector<u8> host(bytes);
    for (int c = 0; c < 2; ++c) {
        memcpy(host.data() + off64[c][0], path[c].data(), path[c].size() * sizeof(u64));
        memcpy(host.data() + off64[c][1], pathB[c].data(), pathB[c].size() * sizeof(u64));
        memcpy(host.data() + off8[c][0], dist[c].data(), dist[c].size());
        memcpy(host.data() + off8[c][1], distB[c].data(), distB[c].size());
    }
    memcpy(host.data() + off_cell, cell.data(), cell.size());
    memcpy(host.data() + off_stab, stab.data(), stab.size());
    memcpy(host.data() + off_ends, ends.data(), ends.size());
    static unsigned long long attr_devs = 0;                          // per device (common.h dq_device_bit)
    const unsigned long long dev_bit = dq_device_bit();
    if (!(attr_devs & dev_bit)) {
        DQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(match_st_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MST_LDS));
        attr_devs |= dev_bit;
    }
    MatchStTables* T = new MatchStTables();
    T->blob = nullptr;
    hipError_t e = hipMalloc(&T->blob, bytes);
    if (e == hipSuccess) e = hipMemcpy(T->blob, host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        dq_set_error("dq_decode_match: table allocation / upload: %s", hipGetErrorString(e));
        match_st_free(T);
        return e == hipErrorOutOfMemory ? DQ_ERR_NOMEM : DQ_ERR_HIP;
    }
    for (int c = 0; c < 2; ++c) {
        T->comp[c].path = reinterpret_cast<const u64*>(T->blob + off64[c][0]);
        T->comp[c].pathB = reinterpret_cast<const u64*>(T->blob + off64[c][1]);
        T->comp[c].dist = T->blob + off8[c][0];
        T->comp[c].distB = T->blob + off8[c][1];
        T->comp[c].n = (int)L.typed[c].size();
    }
    T->cell = T->blob + off_cell;
    T->stab = T->blob + off_stab;
    for (int c = 0; c < 2; ++c) T->uf[c] = UfComp{T->blob + off_ends + 128 * c, T->blob + off_ends + 128 * c + 64, (int)L.typed[c].size(), V->d * V->d};
    V->match_st = T;
    return DQ_OK;
}

extern "C" {

dq_status dq_decode_match(dq_decode_eval* V, const uint8_t* volumes_dev, int n, uint8_t* frame_dev, int32_t* weight_dev, int32_t* n_defects_dev,
                          uint8_t* inexact_dev, void* stream) {
    DQ_REQUIRE(V && volumes_dev && frame_dev, DQ_ERR_INVALID, "dq_decode_match: null argument");
    DQ_REQUIRE(n >= 1 && n <= V->max_volumes, DQ_ERR_INVALID, "dq_decode_match: n = %d outside 1..max_volumes %d", n, V->max_volumes);
    DQ_REQUIRE(((reinterpret_cast<uintptr_t>(weight_dev) | reinterpret_cast<uintptr_t>(n_defects_dev)) & 3) == 0, DQ_ERR_INVALID,
               "dq_decode_match: weight_dev and n_defects_dev must be 4-byte aligned");
    DQ_REQUIRE(V->d <= 7 && V->depth >= 1 && V->depth <= MST_MAX_DEPTH, DQ_ERR_UNSUPPORTED, "dq_decode_match: d = %d, volume_depth = %d: matching covers d <= 7, depth <= %d",
               V->d, V->depth, MST_MAX_DEPTH);
    const dq_status rc = match_st_tables(V);
    if (rc != DQ_OK) return rc;
    const MatchStTables* T = V->match_st;
    match_st_kernel<<<n, 64, MST_LDS, (hipStream_t)stream>>>(T->comp[0], T->comp[1], T->cell, volumes_dev, n, V->d, V->depth, frame_dev, weight_dev, n_defects_dev,
                                                            inexact_dev);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

}  // extern "C"
