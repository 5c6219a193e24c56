// Batched decoding of measured syndrome volumes by a trained agent (include/deepq_hip.h dq_decode_*).
//
// Replaces the reference's "Using a Trained Decoder in Production" loop (README.md:786-829, notebook 3 section 3b), one volume at a time there:
// build the observation, `action = dqn.forward(input_state)`, stop at the identity or a repeated action, otherwise record the action and mark it
// in the action planes.  Here N volumes advance together; per iteration one fused forward over the volumes still decoding (dq_qnet_forward_multi
// with an index gather over the active list) and three small launches of this file:
//   decode_pack_kernel     once per call: grids -> observation rows (patch words or padded uint8 images), the legal set reset_legal_moves builds
//                          from the summed volume (ENV:238-258), empty completed / acted masks, corrections = -1, the identity active list;
//   decode_select_kernel   per iteration: first maximum of each active volume's Q row (common.h's rule with eps = 0, optionally over the legal
//                          set), the step's bookkeeping (ENV:131, 185-201), the action-plane bit of the chosen action set in place, and the number
//                          of volumes that go on per partition of DEC_PART positions;
//   decode_compact_kernel  per iteration: the next active list, stable (a partition's offset is the sum of the counts before it, its volumes
//                          keep their order inside it), and the active count in a device word.
// The host reads that one word per iteration to size the next launches: the only host wait of the loop.
#include "common.h"
#include "qnet.h"
#include "lattice_host.h"
#include "decode_compact.h"

#define DEC_THREADS 256          // select / pack: 16 lanes per volume, 16 volumes per workgroup

namespace {

struct DecTables {
    u64 qubit_cells[64];        // grid cells (row-major over the (d+1)^2 grid, bit r (d+1) + c) of the live stabilizers qubit q touches (ENV:262-271)
    u64 neigh_qmask[64];        // 8-neighbourhood of qubit q (ENV:349-372)
    u8 cell[256];               // padded syndrome plane cell (x, y) of (2d+1)^2: the grid cell copied there (x, y even, ENV:292-294), else 255
    u8 decor[256];              // ... and the constant the embedding puts at the other cells (ENV:284-298)
};

// Per-volume decoding state (written by pack, read and updated by select).
struct DecState {
    u64 legal0, legal1;         // legal_actions (ENV:238-258, 192-196)
    u64 comp0, comp1;           // completed_actions
    u64 acted;                  // acted_on_qubits
    u64 fx, fz;                 // Pauli frame of the recorded corrections: X / Z components (hidden_state codes 1, 2 / 2, 3)
    int32_t n;                  // corrections recorded
    int32_t pad;
};

struct DecArgs {
    const DecTables* tab;
    DecState* state;
    int d, d2, G, P, depth, layers, n_actions, identity, model, use_Y, masked, max_actions, readme, patch;
    int stride_words;           // patch rows: words per row
    int row_bytes;              // uint8 rows: C (2d+1)^2
    void* rows;
    const int32_t* act_in;
    int n_active;
    const float* q;
    int* part;                  // [n / DEC_PART + 1] counts of the volumes that go on, per partition (select adds, compact reads)
    int* part_next;             // the other iteration's counts: compact zeroes them for the next select
    int32_t* act_out;
    int* count;
    const u8* syn;
    int32_t* corr;
    int32_t* n_corr;
    u8* frame;
    u8* status;
};

__device__ __forceinline__ u64 shfl_xor64(u64 v, int m) {
    const u32 lo = __shfl_xor((unsigned)v, m, 16), hi = __shfl_xor((unsigned)(v >> 32), m, 16);
    return (u64)lo | ((u64)hi << 32);
}
__device__ __forceinline__ u64 shfl64(u64 v, int src) {
    const u32 lo = __shfl((unsigned)v, src, 16), hi = __shfl((unsigned)(v >> 32), src, 16);
    return (u64)lo | ((u64)hi << 32);
}
__device__ __forceinline__ u64 group_or(u64 v) {
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v |= shfl_xor64(v, m);
    return v;
}
// (lo, hi) |= v << s over 128 bits, 0 <= s < 128 (env_dev.h or_shl128)
__device__ __forceinline__ void dec_or_shl128(u64& lo, u64& hi, u64 v, int s) {
    lo |= s < 64 ? v << (s & 63) : 0ull;
    hi |= s == 0 ? 0ull : (s < 64 ? v >> ((64 - s) & 63) : v << ((s - 64) & 63));
}

// One volume per 16-lane group.  Lane j < depth gathers slice j into a grid-cell mask; the group ORs them into the summed volume.
__global__ __launch_bounds__(DEC_THREADS) void decode_pack_kernel(DecArgs a, int n) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int v = gid >> 4, sub = gid & 15;
    if (v >= n) return;                                             // whole 16-lane groups leave together
    const DecTables* __restrict__ T = a.tab;
    u64 m = 0;
    if (sub < a.depth) {                                            // G = (d+1)^2 is a multiple of 4: slices are whole aligned words
        const u32* g = reinterpret_cast<const u32*>(a.syn + ((size_t)v * a.depth + sub) * a.G);
        for (int w = 0; w < a.G / 4; ++w) {
            const u32 x = g[w];
#pragma unroll
            for (int b = 0; b < 4; ++b) m |= (u64)(((x >> (8 * b)) & 0xffu) != 0) << (4 * w + b);
        }
    }
    const u64 summed = group_or(m);
    u64 lq = 0;
    for (int q = sub; q < a.d2; q += 16) lq |= (u64)((T->qubit_cells[q] & summed) != 0) << q;
    lq = group_or(lq);
    // ---- observation row ------------------------------------------------------------------------------------------------------
    if (a.patch) {
        u32* row = static_cast<u32*>(a.rows) + (size_t)v * a.stride_words;
        u32 w[4] = {0u, 0u, 0u, 0u};                                // pixels p = sub + 16 k (d^2 <= 49, stride <= 64)
        for (int j = 0; j < a.depth; ++j) {
            const u64 mj = shfl64(m, j);                            // (uniform trip count: every lane of the group shuffles)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = sub + 16 * k;
                if (p < a.d2) {
                    const int oy = p / a.d, ox = p - oy * a.d, c = oy * (a.d + 1) + ox;
                    const u32 bits = (u32)((mj >> c) & 1) | (u32)((mj >> (c + 1)) & 1) << 1 | (u32)((mj >> (c + a.d + 1)) & 1) << 2 |
                                     (u32)((mj >> (c + a.d + 2)) & 1) << 3;       // bit 2 dy + dx <- grid cell (oy + dy, ox + dx)
                    w[k] |= bits << (4 * j);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (sub + 16 * k < a.stride_words) row[sub + 16 * k] = w[k];  // action bits 0, words past d^2 zero
    } else {
        u8* row = static_cast<u8*>(a.rows) + (size_t)v * a.row_bytes;
        const int P2 = a.P * a.P;
        for (int j = 0; j < a.depth; ++j) {
            const u64 mj = shfl64(m, j);
            u8* plane = row + (size_t)j * P2;
            for (int x = sub; x < P2; x += 16) {
                const int c = T->cell[x];
                plane[x] = c != 255 ? (u8)((mj >> c) & 1) : T->decor[x];
            }
        }
        for (int x = a.depth * P2 + sub; x < a.row_bytes; x += 16) row[x] = 0;
    }
    for (int k = sub; k < a.max_actions; k += 16) a.corr[(size_t)v * a.max_actions + k] = -1;
    if (sub == 0) {
        DecState s;
        s.legal0 = s.legal1 = 0;
        dec_or_shl128(s.legal0, s.legal1, 1ull, a.identity);
        for (int j = 0; j < a.layers; ++j) dec_or_shl128(s.legal0, s.legal1, lq, j * a.d2);
        s.comp0 = s.comp1 = 0; s.acted = 0; s.fx = s.fz = 0; s.n = 0; s.pad = 0;
        a.state[v] = s;
        a.n_corr[v] = 0;
        a.status[v] = DQ_DECODE_ACTIVE;
        a.act_out[v] = v;
    }
}

__global__ __launch_bounds__(DEC_THREADS) void decode_select_kernel(DecArgs a) {
    __shared__ int s_keep[DEC_THREADS / 64];
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int g = gid >> 4, sub = gid & 15;
    const bool valid = g < a.n_active;
    const int v = valid ? a.act_in[g] : 0;
    bool keep = false;
    if (valid) {
        DecState s = a.state[v];
        // first maximum of the Q row, over the legal set when masked (common.h's rule with eps = 0); the same in all 16 lanes
        const int act = dq_row_first_max(a.q + (size_t)g * a.n_actions, a.n_actions, sub, dq_admit128(a.masked, s.legal0, s.legal1));
        int st = DQ_DECODE_ACTIVE;
        if (act == a.identity) {
            st = DQ_DECODE_IDENTITY;
        } else if ((((act < 64 ? s.comp0 : s.comp1) >> (act & 63)) & 1)) {
            st = DQ_DECODE_REPEAT;                                  // ENV:131: a repeat is the identity
        } else {
            const int layer = act / a.d2, qb = act - layer * a.d2, i = s.n;
            if (act < 64) s.comp0 |= 1ull << act; else s.comp1 |= 1ull << (act - 64);
            if (!((s.acted >> qb) & 1)) {                           // ENV:190-196
                s.acted |= 1ull << qb;
                for (int j = 0; j < a.layers; ++j) dec_or_shl128(s.legal0, s.legal1, a.tab->neigh_qmask[qb], j * a.d2);
            }
            const int pauli = a.model == DQ_MODEL_X ? 1 : (a.use_Y ? layer + 1 : (layer == 0 ? 1 : 3));     // env.hip: index_to_move
            if (pauli != 3) s.fx ^= 1ull << qb;
            if (pauli != 1) s.fz ^= 1ull << qb;
            s.n = i + 1;
            if (sub == 0) {
                a.corr[(size_t)v * a.max_actions + i] = act;
                // the action-plane cell: the environment marks qubit qb of layer `layer` (ENV:199-201); the README loop writes
                // padding_actions(corrections) into its one action plane, i.e. marks qubit i iff corrections[i] != 0 (README.md:807)
                const int mq = a.readme ? i : qb, ml = a.readme ? 0 : layer;
                const bool on = !a.readme || act != 0;
                if (on) {
                    if (a.patch) {
                        u32* w = static_cast<u32*>(a.rows) + (size_t)v * a.stride_words + mq;
                        *w |= 1u << (4 * a.depth + ml);
                    } else {
                        const int r = mq / a.d, c = mq - r * a.d;
                        static_cast<u8*>(a.rows)[(size_t)v * a.row_bytes + (size_t)(a.depth + ml) * a.P * a.P + (2 * r + 1) * a.P + 2 * c + 1] = 1;
                    }
                }
            }
            if (s.n >= a.max_actions) st = DQ_DECODE_STOPPED;
        }
        if (sub == 0) {
            a.state[v] = s;
            if (st != DQ_DECODE_ACTIVE) { a.status[v] = (u8)st; a.n_corr[v] = s.n; }
        }
        if (st != DQ_DECODE_ACTIVE)
            for (int qb = sub; qb < a.d2; qb += 16) {
                const int x = (int)((s.fx >> qb) & 1), z = (int)((s.fz >> qb) & 1);
                a.frame[(size_t)v * a.d2 + qb] = (u8)(x ? (z ? 2 : 1) : (z ? 3 : 0));
            }
        keep = st == DQ_DECODE_ACTIVE;
    }
    // volumes that go on, counted per workgroup, then added to their partition's count (a workgroup lies inside one partition)
    const u64 bal = __ballot(keep && sub == 0);
    if ((threadIdx.x & 63) == 0) s_keep[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < DEC_THREADS / 64; ++w) c += s_keep[w];
        if (c) atomicAdd(&a.part[(blockIdx.x * (DEC_THREADS / 16)) / DEC_PART], c);
    }
}

// Partition b = positions [b DEC_PART, (b + 1) DEC_PART) of the active list, one per thread (decode_compact.h).
__global__ __launch_bounds__(DEC_PART) void decode_compact_kernel(DecArgs a) {
    decode_compact_partition(a.part, a.part_next, a.act_in, a.n_active, a.status, a.act_out, a.count);
}

}  // namespace

struct dq_decode {
    dq_decode_cfg cfg;
    int max_volumes, layers, n_actions, identity, G, P, row_bytes_u8;
    size_t rows_bytes;
    DecTables* tab;
    DecState* state;
    void* rows;
    int32_t* act[2];
    float* q;
    int* part[2];
    int* count;
    int* count_host;
};

extern "C" {

dq_status dq_decode_create(const dq_decode_cfg* cfg, int max_volumes, dq_decode** out) {
    DQ_REQUIRE(cfg && out, DQ_ERR_INVALID, "dq_decode_create: null argument");
    *out = nullptr;
    DQ_REQUIRE(cfg->d >= 3 && (cfg->d & 1), DQ_ERR_INVALID, "dq_decode_create: d must be odd and >= 3");
    DQ_REQUIRE(cfg->d <= 7, DQ_ERR_UNSUPPORTED, "dq_decode_create: d = %d: decoding covers the one-wavefront lattices, d <= 7", cfg->d);
    DQ_REQUIRE(cfg->volume_depth >= 1 && cfg->volume_depth <= 16, DQ_ERR_INVALID, "dq_decode_create: volume_depth must be in 1..16");
    DQ_REQUIRE(cfg->error_model >= DQ_MODEL_X && cfg->error_model <= DQ_MODEL_IIDXZ, DQ_ERR_INVALID, "dq_decode_create: bad error model");
    DQ_REQUIRE(cfg->action_planes == DQ_DECODE_PLANES_ENV || cfg->action_planes == DQ_DECODE_PLANES_README, DQ_ERR_INVALID,
               "dq_decode_create: bad action-plane mode");
    DQ_REQUIRE(cfg->obs_form == DQ_DECODE_OBS_UINT8 || cfg->obs_form == DQ_DECODE_OBS_PATCH, DQ_ERR_INVALID, "dq_decode_create: bad observation form");
    DQ_REQUIRE(max_volumes >= 1, DQ_ERR_INVALID, "dq_decode_create: max_volumes must be >= 1");
    const int d = cfg->d, d2 = d * d;
    const int layers = cfg->error_model == DQ_MODEL_X ? 1 : (cfg->use_Y ? 3 : 2);
    const int n_actions = layers * d2 + 1;
    DQ_REQUIRE(n_actions <= 128, DQ_ERR_UNSUPPORTED, "dq_decode_create: %d actions: the legal and completed masks hold 128", n_actions);
    DQ_REQUIRE(cfg->max_actions >= 1 && cfg->max_actions <= n_actions - 1, DQ_ERR_INVALID, "dq_decode_create: max_actions must be in 1..%d", n_actions - 1);
    DQ_REQUIRE(cfg->action_planes != DQ_DECODE_PLANES_README || layers == 1, DQ_ERR_INVALID,
               "dq_decode_create: the README action-plane mode is defined for the one action layer of the X model");
    DQ_REQUIRE(cfg->obs_form != DQ_DECODE_OBS_PATCH || 4 * cfg->volume_depth + layers <= 32, DQ_ERR_UNSUPPORTED,
               "dq_decode_create: patch words hold 4 * volume_depth + action layers <= 32 bits");
    DecTables h;
    memset(&h, 0, sizeof(h));
    LatticeHost L;
    lattice_build(d, &L);
    for (int q = 0; q < d2; ++q) {
        for (int s : L.qubit_stabs[q]) h.qubit_cells[q] |= 1ull << (L.sa[s] * (d + 1) + L.sb[s]);
        for (int nb : L.neigh[q]) h.neigh_qmask[q] |= 1ull << nb;
    }
    const int P = 2 * d + 1;
    for (int x = 0; x < P; ++x)
        for (int y = 0; y < P; ++y) {                               // padding_syndrome, ENV:284-298
            int c = 255, s = 0;
            if ((x == 0 || x == 2 * d) && (y & 1)) s = 1;
            if ((y == 0 || y == 2 * d) && (x & 1)) s = 1;
            if (!(x & 1) && !(y & 1)) c = (x / 2) * (d + 1) + y / 2;
            else if ((x & 1) && (y & 1) && (x + y) % 4 == 0) s = 1;
            h.cell[x * P + y] = (u8)c;
            h.decor[x * P + y] = (u8)s;
        }
    dq_decode* D = new dq_decode();
    memset(D, 0, sizeof(*D));
    D->cfg = *cfg; D->max_volumes = max_volumes; D->layers = layers; D->n_actions = n_actions; D->identity = n_actions - 1;
    D->G = (d + 1) * (d + 1); D->P = P; D->row_bytes_u8 = (cfg->volume_depth + layers) * P * P;
    const size_t row = cfg->obs_form == DQ_DECODE_OBS_PATCH ? 64 * sizeof(u32) : (size_t)D->row_bytes_u8;
    D->rows_bytes = ((size_t)max_volumes * row + 15) / 16 * 16;
    const int parts = max_volumes / DEC_PART + 1;
    hipError_t e = hipMalloc(&D->tab, sizeof(DecTables));
    if (e == hipSuccess) e = hipMemcpy(D->tab, &h, sizeof(DecTables), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&D->state, (size_t)max_volumes * sizeof(DecState));
    if (e == hipSuccess) e = hipMalloc(&D->rows, D->rows_bytes);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipMalloc(&D->act[i], (size_t)max_volumes * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&D->q, (size_t)max_volumes * n_actions * sizeof(float));
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipMalloc(&D->part[i], (size_t)parts * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&D->count, sizeof(int));
    if (e == hipSuccess) e = hipHostMalloc(&D->count_host, sizeof(int), hipHostMallocDefault);
    if (e != hipSuccess) {
        dq_set_error("dq_decode_create: %s", hipGetErrorString(e));
        dq_decode_destroy(D);
        return e == hipErrorOutOfMemory ? DQ_ERR_NOMEM : DQ_ERR_HIP;
    }
    *out = D;
    return DQ_OK;
}

void dq_decode_destroy(dq_decode* D) {
    if (!D) return;
    if (D->tab) (void)hipFree(D->tab);
    if (D->state) (void)hipFree(D->state);
    if (D->rows) (void)hipFree(D->rows);
    for (int i = 0; i < 2; ++i) if (D->act[i]) (void)hipFree(D->act[i]);
    if (D->q) (void)hipFree(D->q);
    for (int i = 0; i < 2; ++i) if (D->part[i]) (void)hipFree(D->part[i]);
    if (D->count) (void)hipFree(D->count);
    if (D->count_host) (void)hipHostFree(D->count_host);
    delete D;
}

dq_status dq_decode_run(dq_decode* D, dq_qnet* net, const float* params_dev, const void* packed_dev, const uint8_t* syndromes_dev, int n,
                        int32_t* corrections_dev, int32_t* n_corr_dev, uint8_t* frame_dev, uint8_t* status_dev, int* iterations, void* stream) {
    DQ_REQUIRE(D && net && params_dev && syndromes_dev && corrections_dev && n_corr_dev && frame_dev && status_dev, DQ_ERR_INVALID,
               "dq_decode_run: null argument");
    const dq_decode_cfg& c = D->cfg;
    const int d = c.d, P = D->P;
    DQ_REQUIRE(n >= 1 && n <= D->max_volumes && n <= net->cfg.max_batch, DQ_ERR_INVALID,
               "dq_decode_run: n = %d outside 1..min(max_volumes %d, the network's max_batch %d)", n, D->max_volumes, net->cfg.max_batch);
    DQ_REQUIRE(net->cfg.n_actions == D->n_actions && net->cfg.in_c == c.volume_depth + D->layers && net->cfg.in_h == P && net->cfg.in_w == P,
               DQ_ERR_INVALID, "dq_decode_run: the network's input (%d, %d, %d) -> %d actions does not fit the lattice (%d, %d, %d) -> %d",
               net->cfg.in_c, net->cfg.in_h, net->cfg.in_w, net->cfg.n_actions, c.volume_depth + D->layers, P, P, D->n_actions);
    DQ_REQUIRE((reinterpret_cast<uintptr_t>(syndromes_dev) & 3) == 0, DQ_ERR_INVALID, "dq_decode_run: syndromes_dev must be 4-byte aligned");
    const bool patch = c.obs_form == DQ_DECODE_OBS_PATCH;
    if (patch)
        DQ_REQUIRE(net->patch_depth == c.volume_depth && net->patch_stride >= d * d && net->patch_stride <= 64, DQ_ERR_STATE,
                   "dq_decode_run: patch-word decoding needs dq_qnet_set_patch_input(net, %d, stride) on the network", c.volume_depth);
    hipStream_t st = (hipStream_t)stream;
    DecArgs a;
    memset(&a, 0, sizeof(a));
    a.tab = D->tab; a.state = D->state; a.d = d; a.d2 = d * d; a.G = D->G; a.P = P; a.depth = c.volume_depth; a.layers = D->layers;
    a.n_actions = D->n_actions; a.identity = D->identity; a.model = c.error_model; a.use_Y = c.use_Y ? 1 : 0; a.masked = c.masked_greedy ? 1 : 0;
    a.max_actions = c.max_actions; a.readme = c.action_planes == DQ_DECODE_PLANES_README; a.patch = patch ? 1 : 0;
    a.stride_words = patch ? net->patch_stride : 0; a.row_bytes = D->row_bytes_u8; a.rows = D->rows;
    a.syn = syndromes_dev; a.corr = corrections_dev; a.n_corr = n_corr_dev; a.frame = frame_dev; a.status = status_dev; a.count = D->count;
    a.act_out = D->act[0];                                          // (pack: the identity active list)
    const int parts = n / DEC_PART + 1;
    DQ_HIP(hipMemsetAsync(D->part[0], 0, (size_t)parts * sizeof(int), st));
    DQ_HIP(hipMemsetAsync(D->part[1], 0, (size_t)parts * sizeof(int), st));
    decode_pack_kernel<<<(n * 16 + DEC_THREADS - 1) / DEC_THREADS, DEC_THREADS, 0, st>>>(a, n);
    DQ_LAUNCH_CHECK();
    int n_active = n, it = 0, cur = 0;
    while (n_active > 0) {
        DQ_REQUIRE(it < c.max_actions, DQ_ERR_STATE, "dq_decode_run: volumes still active after max_actions iterations");
        dq_qnet_job jb;
        memset(&jb, 0, sizeof(jb));
        jb.params_dev = params_dev; jb.obs_dev = static_cast<const uint8_t*>(D->rows); jb.index_dev = D->act[cur]; jb.batch = n_active;
        jb.reserved = patch ? 1u : 0u; jb.q_dev = D->q; jb.packed_dev = packed_dev;
        dq_status rc = dq_qnet_forward_multi(net, 1, &jb, stream);
        if (rc != DQ_OK) return rc;
        a.act_in = D->act[cur]; a.act_out = D->act[cur ^ 1]; a.n_active = n_active; a.q = D->q;
        a.part = D->part[it & 1]; a.part_next = D->part[(it + 1) & 1];
        decode_select_kernel<<<(n_active * 16 + DEC_THREADS - 1) / DEC_THREADS, DEC_THREADS, 0, st>>>(a);
        DQ_LAUNCH_CHECK();
        decode_compact_kernel<<<(n_active + DEC_PART - 1) / DEC_PART, DEC_PART, 0, st>>>(a);
        DQ_LAUNCH_CHECK();
        DQ_HIP(hipMemcpyAsync(D->count_host, D->count, sizeof(int), hipMemcpyDeviceToHost, st));
        DQ_HIP(hipStreamSynchronize(st));                          // the loop's one host wait: the next grid's size
        const int next = *D->count_host;
        DQ_REQUIRE(next >= 0 && next <= n_active, DQ_ERR_STATE, "dq_decode_run: active count %d after %d", next, n_active);
        n_active = next;
        cur ^= 1;
        ++it;
    }
    if (iterations) *iterations = it;
    // a non-finite forward must not pass as a chosen correction: the forward's range guard reports it here (dq_qnet_range_check[forward])
    return dq_qnet_range_check(net, stream);
}

}  // extern "C"
