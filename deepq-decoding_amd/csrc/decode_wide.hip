// Batched decoding of measured syndrome volumes by a trained agent for any odd d in 3 .. 15 (include/deepq_hip.h dq_decode_wide_*).
//
// The loop and its semantics are decode.hip's (README.md:786-829; Environments.py:131, 185-201, 238-271), with the environment's action planes and uint8
// observation rows.  What differs is the state: up to 3 * 225 + 1 = 676 actions, so the legal and the completed set are LW = ceil(num_actions / 64) <= 11
// words each, the acted-on qubits and the two frame components ceil(d^2 / 64) <= 4 words each, a slice's grid mask ceil((d+1)^2 / 64) <= 4 words (at
// d = 15 the grid is exactly 256 cells).  One wavefront per volume; a multi-word set lives one word per lane (lane w holds word w), so no thread indexes
// a register array: a word of another lane comes by v_readlane (wave-uniform index) or a shuffle, and a multi-word shift is two shuffles per lane.
//   decode_wide_pack_kernel     once per call: the depth slices -> grid words (one ballot per 64 cells) in LDS and their OR; the legal set of
//                               reset_legal_moves through the qubit -> grid-cell table; the padded row (depth + layers) (2d+1)^2 bytes in 16-byte stores,
//                               the action planes zero; corrections = -1, the empty state, the identity active list;
//   decode_wide_select_kernel   per iteration: first maximum of each active volume's Q row (common.h's rule at eps = 0: the lowest index
//                               among equal maxima, over the legal words when masked), the step's bookkeeping, the one action-plane byte set in place, the
//                               per-partition keep counts, and a sticky device word where a Q of the row is not finite;
//   decode_wide_compact_kernel  decode_compact.h's rule, as in decode.hip.
#include "common.h"
#include "qnet.h"
#include "lattice_host.h"
#include "decode_compact.h"

#define DW_THREADS 256           // four wavefronts = four volumes per workgroup
#define DW_WAVES (DW_THREADS / 64)
#define DW_MAX_D 15
#define DW_MAX_Q (DW_MAX_D * DW_MAX_D)                   // 225 qubits
#define DW_QW 4                                          // words of a qubit set / of a slice's grid mask
#define DW_LW 11                                         // words of an action set at most
#define DW_MAX_DEPTH 16
#define DW_MAX_P2 ((2 * DW_MAX_D + 1) * (2 * DW_MAX_D + 1))   // 961 cells of a padded plane
#define DW_NO_CELL 0x1ff

namespace {

struct WTables {
    u64 qubit_cells[DW_MAX_Q][DW_QW];   // grid cells (row-major over the (d+1)^2 grid) of the live stabilizers qubit q touches (ENV:262-271)
    u64 neigh[DW_MAX_Q][DW_QW];         // 8-neighbourhood of qubit q (ENV:349-372)
    uint16_t emb[DW_MAX_P2 + 3];        // padded plane cell x: bits 0..8 the grid cell copied there (ENV:292-294) or DW_NO_CELL, bit 15 the constant
};                                      // the embedding puts there otherwise (ENV:284-298)

struct WArgs {
    const WTables* tab;
    u64* legal;                 // [max_volumes][LW]  legal_actions (ENV:238-258, 192-196)
    u64* comp;                  // [max_volumes][LW]  completed_actions
    u64* misc;                  // [max_volumes][3][DW_QW]  acted_on_qubits, frame X component, frame Z component
    int* cnt;                   // [max_volumes]  corrections recorded
    u8* rows;
    int d, d2, G, P2, depth, layers, n_actions, identity, model, use_Y, masked, max_actions, LW, row_bytes;
    const int32_t* act_in;
    int n_active;
    const float* q;
    int* part;
    int* part_next;
    int32_t* act_out;
    int* count;                 // [0] the active count, [1] the sticky non-finite word
    const u8* syn;
    int32_t* corr;
    int32_t* n_corr;
    u8* frame;
    u8* status;
};

__device__ __forceinline__ u64 dw_shfl64(u64 v, int src) {
    const u32 lo = __shfl((unsigned)v, src), hi = __shfl((unsigned)(v >> 32), src);
    return (u64)lo | ((u64)hi << 32);
}
// Word `lane` of (V << s), V the multi-word value whose word w lane w holds in v (0 in the lanes past its last word); every lane calls.
__device__ __forceinline__ u64 dw_shl_word(u64 v, int s, int lane) {
    const int idx = lane - (s >> 6), r = s & 63;
    const u64 lo = dw_shfl64(v, idx & 63), hi = dw_shfl64(v, (idx - 1) & 63);
    return (idx >= 0 ? lo << r : 0ull) | (r != 0 && idx >= 1 ? hi >> (64 - r) : 0ull);
}

// Byte x of volume's padded row: plane `plane` < depth reads the slice's grid mask, the action planes start empty.
__device__ __forceinline__ u32 dw_row_byte(const uint16_t* emb, const u64* m, int plane, int pos, int depth) {
    if (plane >= depth) return 0u;
    const u32 e = emb[pos], c = e & 0x1ffu;
    return c != DW_NO_CELL ? (u32)((m[plane * DW_QW + (c >> 6)] >> (c & 63)) & 1) : e >> 15;
}

__global__ __launch_bounds__(DW_THREADS) void decode_wide_pack_kernel(WArgs a, int n) {
    __shared__ uint16_t s_emb[DW_MAX_P2 + 3];
    __shared__ u64 s_m[DW_WAVES][DW_MAX_DEPTH * DW_QW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int v = blockIdx.x * DW_WAVES + wave;
    const bool active = v < n;                                      // wave-uniform
    const WTables* __restrict__ T = a.tab;
    for (int x = threadIdx.x; x < a.P2; x += DW_THREADS) s_emb[x] = T->emb[x];
    u64 summed[DW_QW] = {0ull, 0ull, 0ull, 0ull};
    u64* m = s_m[wave];
    if (active) {
        for (int j = 0; j < a.depth; ++j) {
            const u8* g = a.syn + ((size_t)v * a.depth + j) * a.G;
#pragma unroll
            for (int w = 0; w < DW_QW; ++w) {
                const int c = 64 * w + lane;
                const u64 bits = __ballot(c < a.G && g[c] != 0);
                summed[w] |= bits;
                if (lane == 0) m[j * DW_QW + w] = bits;
            }
        }
    }
    __syncthreads();                                                // the embedding table and the wave's grid masks are in LDS
    if (!active) return;
    // ---- the legal set: reset_legal_moves of the summed volume (ENV:238-271) ---------------------------------------------------------
    u64 lqv = 0;                                                    // lane k < DW_QW: word k of the set of qubits next to a live cell
#pragma unroll
    for (int k = 0; k < DW_QW; ++k) {
        const int qb = 64 * k + lane;
        bool hit = false;
        if (qb < a.d2) {
#pragma unroll
            for (int w = 0; w < DW_QW; ++w) hit |= (T->qubit_cells[qb][w] & summed[w]) != 0;
        }
        const u64 bits = __ballot(hit);
        if (lane == k) lqv = bits;
    }
    u64 legal = 0;
    for (int j = 0; j < a.layers; ++j) legal |= dw_shl_word(lqv, j * a.d2, lane);
    if (lane == (a.identity >> 6)) legal |= 1ull << (a.identity & 63);
    if (lane < a.LW) {
        a.legal[(size_t)v * a.LW + lane] = legal;
        a.comp[(size_t)v * a.LW + lane] = 0;
    }
    if (lane < 3 * DW_QW) a.misc[(size_t)v * (3 * DW_QW) + lane] = 0;
    for (int k = lane; k < a.max_actions; k += 64) a.corr[(size_t)v * a.max_actions + k] = -1;
    if (lane == 0) {
        a.cnt[v] = 0;
        a.n_corr[v] = 0;
        a.status[v] = DQ_DECODE_ACTIVE;
        a.act_out[v] = v;
    }
    // ---- the observation row: head bytes up to the first 16-byte boundary, 16-byte stores, tail bytes -------------------------------------
    u8* row = a.rows + (size_t)v * a.row_bytes;
    int head = (int)((16u - (u32)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u);
    if (head > a.row_bytes) head = a.row_bytes;
    if (lane < head) {
        const int plane = lane / a.P2;
        row[lane] = (u8)dw_row_byte(s_emb, m, plane, lane - plane * a.P2, a.depth);
    }
    const int nvec = (a.row_bytes - head) >> 4;
    for (int t = lane; t < nvec; t += 64) {
        const int x0 = head + 16 * t;
        int plane = x0 / a.P2, pos = x0 - plane * a.P2;
        u32 w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            u32 word = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                word |= dw_row_byte(s_emb, m, plane, pos, a.depth) << (8 * b);
                if (++pos == a.P2) { pos = 0; ++plane; }
            }
            w[i] = word;
        }
        *reinterpret_cast<uint4*>(row + x0) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    const int x = head + 16 * nvec + lane;                          // (fewer than 16 bytes are left)
    if (x < a.row_bytes) {
        const int plane = x / a.P2;
        row[x] = (u8)dw_row_byte(s_emb, m, plane, x - plane * a.P2, a.depth);
    }
}

__global__ __launch_bounds__(DW_THREADS) void decode_wide_select_kernel(WArgs a) {
    __shared__ int s_keep[DW_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * DW_WAVES + wave;
    bool keep = false;
    if (g < a.n_active) {                                           // wave-uniform: the whole wavefront works on volume v
        const int v = __builtin_amdgcn_readfirstlane(a.act_in[g]);
        u64 legal = 0, comp = 0, acted = 0, fx = 0, fz = 0;         // lane w: word w of each set
        if (lane < a.LW) { legal = a.legal[(size_t)v * a.LW + lane]; comp = a.comp[(size_t)v * a.LW + lane]; }
        u64* misc = a.misc + (size_t)v * (3 * DW_QW);
        if (lane < DW_QW) { acted = misc[lane]; fx = misc[DW_QW + lane]; fz = misc[2 * DW_QW + lane]; }
        int cnt = a.cnt[v];
        // first maximum of the Q row, over the legal words when masked (common.h's rule with eps = 0; wave-uniform); word j of the set comes from lane j
        bool bad = false;
        int act = dq_wave_first_max(a.q + (size_t)g * a.n_actions, a.n_actions, lane,
                                    dq_admit_words(a.masked, [=](int j) { return wave_bcast64(legal, __builtin_amdgcn_readfirstlane(j)); }),
                                    [&](float x) { bad |= !(fabsf(x) < INFINITY); });                // NaN fails the compare too
        int st = DQ_DECODE_ACTIVE;
        if ((unsigned)act >= (unsigned)a.n_actions) { bad = true; act = a.identity; }      // (no candidate: the identity is always one)
        if (act == a.identity) {
            st = DQ_DECODE_IDENTITY;
        } else if ((wave_bcast64(comp, act >> 6) >> (act & 63)) & 1) {
            st = DQ_DECODE_REPEAT;                                  // ENV:131: a repeat is the identity
        } else {
            const int layer = act / a.d2, qb = act - layer * a.d2;
            if (lane == (act >> 6)) comp |= 1ull << (act & 63);
            if (!((wave_bcast64(acted, qb >> 6) >> (qb & 63)) & 1)) {                       // ENV:190-196
                if (lane == (qb >> 6)) acted |= 1ull << (qb & 63);
                const u64 nv = lane < DW_QW ? a.tab->neigh[qb][lane] : 0ull;
                for (int j = 0; j < a.layers; ++j) legal |= dw_shl_word(nv, j * a.d2, lane);
            }
            const int pauli = a.model == DQ_MODEL_X ? 1 : (a.use_Y ? layer + 1 : (layer == 0 ? 1 : 3));     // env.hip: index_to_move
            if (lane == (qb >> 6)) {
                if (pauli != 3) fx ^= 1ull << (qb & 63);
                if (pauli != 1) fz ^= 1ull << (qb & 63);
            }
            if (lane == 0) {
                a.corr[(size_t)v * a.max_actions + cnt] = act;
                const int r = qb / a.d, c = qb - r * a.d, P = 2 * a.d + 1;                  // ENV:199-201
                a.rows[(size_t)v * a.row_bytes + (size_t)(a.depth + layer) * a.P2 + (2 * r + 1) * P + 2 * c + 1] = 1;
            }
            ++cnt;
            if (cnt >= a.max_actions) st = DQ_DECODE_STOPPED;
        }
        if (lane < a.LW) { a.legal[(size_t)v * a.LW + lane] = legal; a.comp[(size_t)v * a.LW + lane] = comp; }
        if (lane < DW_QW) { misc[lane] = acted; misc[DW_QW + lane] = fx; misc[2 * DW_QW + lane] = fz; }
        if (lane == 0) {
            a.cnt[v] = cnt;
            if (st != DQ_DECODE_ACTIVE) { a.status[v] = (u8)st; a.n_corr[v] = cnt; }
        }
        if (st != DQ_DECODE_ACTIVE) {
#pragma unroll
            for (int k = 0; k < DW_QW; ++k) {
                const u64 wx = wave_bcast64(fx, k), wz = wave_bcast64(fz, k);
                const int qb = 64 * k + lane;
                if (qb < a.d2) {
                    const int x = (int)((wx >> lane) & 1), z = (int)((wz >> lane) & 1);
                    a.frame[(size_t)v * a.d2 + qb] = (u8)(x ? (z ? 2 : 1) : (z ? 3 : 0));
                }
            }
        }
        if (__ballot(bad) != 0 && lane == 0) atomicOr(reinterpret_cast<unsigned*>(a.count) + 1, 1u);
        keep = st == DQ_DECODE_ACTIVE;
    }
    // volumes that go on, counted per workgroup, then added to their partition's count (a workgroup lies inside one partition)
    if (lane == 0) s_keep[wave] = keep ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < DW_WAVES; ++w) c += s_keep[w];
        if (c) atomicAdd(&a.part[(blockIdx.x * DW_WAVES) / DEC_PART], c);
    }
}

__global__ __launch_bounds__(DEC_PART) void decode_wide_compact_kernel(WArgs a) {
    decode_compact_partition(a.part, a.part_next, a.act_in, a.n_active, a.status, a.act_out, a.count);
}

}  // namespace

struct dq_decode_wide {
    dq_decode_cfg cfg;
    int max_volumes, layers, n_actions, identity, G, P, row_bytes, LW;
    WTables* tab;
    u64* legal;
    u64* comp;
    u64* misc;
    int* cnt;
    u8* rows;
    int32_t* act[2];
    float* q;
    int* part[2];
    int* count;                 // two words: the active count, the sticky non-finite word
    int* count_host;
    // the decode in flight (dq_decode_wide_pack .. the step that leaves no volume active)
    int n, n_active, it, cur;
    int32_t* corr;
    int32_t* n_corr;
    u8* frame;
    u8* status;
};

static void dw_args(const dq_decode_wide* D, WArgs* a) {
    memset(a, 0, sizeof(*a));
    const dq_decode_cfg& c = D->cfg;
    a->tab = D->tab; a->legal = D->legal; a->comp = D->comp; a->misc = D->misc; a->cnt = D->cnt; a->rows = D->rows;
    a->d = c.d; a->d2 = c.d * c.d; a->G = D->G; a->P2 = D->P * D->P; a->depth = c.volume_depth; a->layers = D->layers; a->n_actions = D->n_actions;
    a->identity = D->identity; a->model = c.error_model; a->use_Y = c.use_Y ? 1 : 0; a->masked = c.masked_greedy ? 1 : 0; a->max_actions = c.max_actions;
    a->LW = D->LW; a->row_bytes = D->row_bytes; a->count = D->count;
    a->corr = D->corr; a->n_corr = D->n_corr; a->frame = D->frame; a->status = D->status;
}

static dq_status dw_pack(dq_decode_wide* D, const uint8_t* syndromes_dev, int n, int32_t* corrections_dev, int32_t* n_corr_dev, uint8_t* frame_dev,
                         uint8_t* status_dev, hipStream_t st, const char* who) {
    DQ_REQUIRE(syndromes_dev && corrections_dev && n_corr_dev && frame_dev && status_dev, DQ_ERR_INVALID, "%s: null argument", who);
    DQ_REQUIRE(n >= 1 && n <= D->max_volumes, DQ_ERR_INVALID, "%s: n = %d outside 1..max_volumes %d", who, n, D->max_volumes);
    DQ_REQUIRE((reinterpret_cast<uintptr_t>(syndromes_dev) & 3) == 0, DQ_ERR_INVALID, "%s: syndromes_dev must be 4-byte aligned", who);
    D->n = 0; D->n_active = 0;
    D->corr = corrections_dev; D->n_corr = n_corr_dev; D->frame = frame_dev; D->status = status_dev;
    WArgs a;
    dw_args(D, &a);
    a.syn = syndromes_dev; a.act_out = D->act[0];
    const int parts = n / DEC_PART + 1;
    DQ_HIP(hipMemsetAsync(D->part[0], 0, (size_t)parts * sizeof(int), st));
    DQ_HIP(hipMemsetAsync(D->part[1], 0, (size_t)parts * sizeof(int), st));
    DQ_HIP(hipMemsetAsync(D->count, 0, 2 * sizeof(int), st));
    decode_wide_pack_kernel<<<(n + DW_WAVES - 1) / DW_WAVES, DW_THREADS, 0, st>>>(a, n);
    DQ_LAUNCH_CHECK();
    D->n = n; D->n_active = n; D->it = 0; D->cur = 0;
    return DQ_OK;
}

static dq_status dw_step(dq_decode_wide* D, const float* q_dev, hipStream_t st, const char* who) {
    DQ_REQUIRE(q_dev, DQ_ERR_INVALID, "%s: null Q rows", who);
    DQ_REQUIRE((reinterpret_cast<uintptr_t>(q_dev) & 3) == 0, DQ_ERR_INVALID, "%s: q_dev must be 4-byte aligned", who);
    DQ_REQUIRE(D->n >= 1 && D->n_active >= 1, DQ_ERR_STATE, "%s: no volume is decoding (dq_decode_wide_pack starts a decode)", who);
    DQ_REQUIRE(D->it < D->cfg.max_actions, DQ_ERR_STATE, "%s: volumes still active after max_actions iterations", who);
    WArgs a;
    dw_args(D, &a);
    const int n_active = D->n_active;
    a.act_in = D->act[D->cur]; a.act_out = D->act[D->cur ^ 1]; a.n_active = n_active; a.q = q_dev;
    a.part = D->part[D->it & 1]; a.part_next = D->part[(D->it + 1) & 1];
    decode_wide_select_kernel<<<(n_active + DW_WAVES - 1) / DW_WAVES, DW_THREADS, 0, st>>>(a);
    DQ_LAUNCH_CHECK();
    decode_wide_compact_kernel<<<(n_active + DEC_PART - 1) / DEC_PART, DEC_PART, 0, st>>>(a);
    DQ_LAUNCH_CHECK();
    DQ_HIP(hipMemcpyAsync(D->count_host, D->count, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    DQ_HIP(hipStreamSynchronize(st));                              // the iteration's one host wait: the next grid's size and the sticky word
    const int next = D->count_host[0];
    if (D->count_host[1] != 0) {
        D->n = 0; D->n_active = 0;
        dq_set_error("%s: a Q-value of iteration %d is not finite: a non-finite forward must not pass as a chosen correction", who, D->it);
        return DQ_ERR_RANGE;
    }
    DQ_REQUIRE(next >= 0 && next <= n_active, DQ_ERR_STATE, "%s: active count %d after %d", who, next, n_active);
    D->n_active = next;
    D->cur ^= 1;
    ++D->it;
    return DQ_OK;
}

extern "C" {

dq_status dq_decode_wide_create(const dq_decode_cfg* cfg, int max_volumes, dq_decode_wide** out) {
    DQ_REQUIRE(cfg && out, DQ_ERR_INVALID, "dq_decode_wide_create: null argument");
    *out = nullptr;
    DQ_REQUIRE(cfg->d >= 3 && cfg->d <= DW_MAX_D && (cfg->d & 1), DQ_ERR_INVALID, "dq_decode_wide_create: d must be odd and in 3..%d", DW_MAX_D);
    DQ_REQUIRE(cfg->volume_depth >= 1 && cfg->volume_depth <= DW_MAX_DEPTH, DQ_ERR_INVALID, "dq_decode_wide_create: volume_depth must be in 1..%d",
               DW_MAX_DEPTH);
    DQ_REQUIRE(cfg->error_model >= DQ_MODEL_X && cfg->error_model <= DQ_MODEL_IIDXZ, DQ_ERR_INVALID, "dq_decode_wide_create: bad error model");
    DQ_REQUIRE(cfg->action_planes == DQ_DECODE_PLANES_ENV, DQ_ERR_UNSUPPORTED,
               "dq_decode_wide_create: the environment's action planes only (the README mode is dq_decode_create's)");
    DQ_REQUIRE(cfg->obs_form == DQ_DECODE_OBS_UINT8, DQ_ERR_UNSUPPORTED, "dq_decode_wide_create: uint8 observation rows only (patch words are dq_decode_create's)");
    DQ_REQUIRE(max_volumes >= 1, DQ_ERR_INVALID, "dq_decode_wide_create: max_volumes must be >= 1");
    const int d = cfg->d, d2 = d * d;
    const int layers = cfg->error_model == DQ_MODEL_X ? 1 : (cfg->use_Y ? 3 : 2);
    const int n_actions = layers * d2 + 1;
    DQ_REQUIRE(cfg->max_actions >= 1 && cfg->max_actions <= n_actions - 1, DQ_ERR_INVALID, "dq_decode_wide_create: max_actions must be in 1..%d",
               n_actions - 1);
    WTables* h = new WTables();
    memset(h, 0, sizeof(*h));
    LatticeHost L;
    lattice_build(d, &L);
    for (int q = 0; q < d2; ++q) {
        for (int s : L.qubit_stabs[q]) { const int c = L.sa[s] * (d + 1) + L.sb[s]; h->qubit_cells[q][c >> 6] |= 1ull << (c & 63); }
        for (int nb : L.neigh[q]) h->neigh[q][nb >> 6] |= 1ull << (nb & 63);
    }
    const int P = 2 * d + 1;
    for (int x = 0; x < P; ++x)
        for (int y = 0; y < P; ++y) {                               // padding_syndrome, ENV:284-298
            int c = DW_NO_CELL, s = 0;
            if ((x == 0 || x == 2 * d) && (y & 1)) s = 1;
            if ((y == 0 || y == 2 * d) && (x & 1)) s = 1;
            if (!(x & 1) && !(y & 1)) c = (x / 2) * (d + 1) + y / 2;
            else if ((x & 1) && (y & 1) && (x + y) % 4 == 0) s = 1;
            h->emb[x * P + y] = (uint16_t)(c | (s << 15));
        }
    dq_decode_wide* D = new dq_decode_wide();
    memset(D, 0, sizeof(*D));
    D->cfg = *cfg; D->max_volumes = max_volumes; D->layers = layers; D->n_actions = n_actions; D->identity = n_actions - 1;
    D->G = (d + 1) * (d + 1); D->P = P; D->row_bytes = (cfg->volume_depth + layers) * P * P; D->LW = (n_actions + 63) / 64;
    const size_t nv = (size_t)max_volumes;
    const int parts = max_volumes / DEC_PART + 1;
    hipError_t e = hipMalloc(&D->tab, sizeof(WTables));
    if (e == hipSuccess) e = hipMemcpy(D->tab, h, sizeof(WTables), hipMemcpyHostToDevice);
    delete h;
    if (e == hipSuccess) e = hipMalloc(&D->legal, nv * D->LW * sizeof(u64));
    if (e == hipSuccess) e = hipMalloc(&D->comp, nv * D->LW * sizeof(u64));
    if (e == hipSuccess) e = hipMalloc(&D->misc, nv * 3 * DW_QW * sizeof(u64));
    if (e == hipSuccess) e = hipMalloc(&D->cnt, nv * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&D->rows, (nv * D->row_bytes + 15) / 16 * 16);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipMalloc(&D->act[i], nv * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&D->q, nv * n_actions * sizeof(float));
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipMalloc(&D->part[i], (size_t)parts * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&D->count, 2 * sizeof(int));
    if (e == hipSuccess) e = hipHostMalloc(&D->count_host, 2 * sizeof(int), hipHostMallocDefault);
    if (e != hipSuccess) {
        dq_set_error("dq_decode_wide_create: %s", hipGetErrorString(e));
        dq_decode_wide_destroy(D);
        return e == hipErrorOutOfMemory ? DQ_ERR_NOMEM : DQ_ERR_HIP;
    }
    *out = D;
    return DQ_OK;
}

void dq_decode_wide_destroy(dq_decode_wide* D) {
    if (!D) return;
    if (D->tab) (void)hipFree(D->tab);
    if (D->legal) (void)hipFree(D->legal);
    if (D->comp) (void)hipFree(D->comp);
    if (D->misc) (void)hipFree(D->misc);
    if (D->cnt) (void)hipFree(D->cnt);
    if (D->rows) (void)hipFree(D->rows);
    for (int i = 0; i < 2; ++i) if (D->act[i]) (void)hipFree(D->act[i]);
    if (D->q) (void)hipFree(D->q);
    for (int i = 0; i < 2; ++i) if (D->part[i]) (void)hipFree(D->part[i]);
    if (D->count) (void)hipFree(D->count);
    if (D->count_host) (void)hipHostFree(D->count_host);
    delete D;
}

dq_status dq_decode_wide_pack(dq_decode_wide* D, const uint8_t* syndromes_dev, int n, int32_t* corrections_dev, int32_t* n_corr_dev, uint8_t* frame_dev,
                              uint8_t* status_dev, void* stream) {
    DQ_REQUIRE(D, DQ_ERR_INVALID, "dq_decode_wide_pack: null handle");
    return dw_pack(D, syndromes_dev, n, corrections_dev, n_corr_dev, frame_dev, status_dev, (hipStream_t)stream, "dq_decode_wide_pack");
}

dq_status dq_decode_wide_step(dq_decode_wide* D, const float* q_dev, int* n_active_out, void* stream) {
    DQ_REQUIRE(D, DQ_ERR_INVALID, "dq_decode_wide_step: null handle");
    const dq_status rc = dw_step(D, q_dev, (hipStream_t)stream, "dq_decode_wide_step");
    if (rc == DQ_OK && n_active_out) *n_active_out = D->n_active;
    return rc;
}

dq_status dq_decode_wide_run(dq_decode_wide* D, dq_qnet* net, const float* params_dev, const void* packed_dev, const uint8_t* syndromes_dev, int n,
                             int32_t* corrections_dev, int32_t* n_corr_dev, uint8_t* frame_dev, uint8_t* status_dev, int* iterations, void* stream) {
    DQ_REQUIRE(D && net && params_dev, DQ_ERR_INVALID, "dq_decode_wide_run: null argument");
    const dq_decode_cfg& c = D->cfg;
    const int P = D->P;
    DQ_REQUIRE(n >= 1 && n <= D->max_volumes && n <= net->cfg.max_batch, DQ_ERR_INVALID,
               "dq_decode_wide_run: n = %d outside 1..min(max_volumes %d, the network's max_batch %d)", n, D->max_volumes, net->cfg.max_batch);
    DQ_REQUIRE(net->cfg.n_actions == D->n_actions && net->cfg.in_c == c.volume_depth + D->layers && net->cfg.in_h == P && net->cfg.in_w == P,
               DQ_ERR_INVALID, "dq_decode_wide_run: the network's input (%d, %d, %d) -> %d actions does not fit the lattice (%d, %d, %d) -> %d",
               net->cfg.in_c, net->cfg.in_h, net->cfg.in_w, net->cfg.n_actions, c.volume_depth + D->layers, P, P, D->n_actions);
    dq_status rc = dw_pack(D, syndromes_dev, n, corrections_dev, n_corr_dev, frame_dev, status_dev, (hipStream_t)stream, "dq_decode_wide_run");
    if (rc != DQ_OK) return rc;
    while (D->n_active > 0) {
        dq_qnet_job jb;
        memset(&jb, 0, sizeof(jb));
        jb.params_dev = params_dev; jb.obs_dev = D->rows; jb.index_dev = D->act[D->cur]; jb.batch = D->n_active;
        jb.q_dev = D->q; jb.packed_dev = packed_dev;
        rc = dq_qnet_forward_multi(net, 1, &jb, stream);
        if (rc != DQ_OK) return rc;
        rc = dw_step(D, D->q, (hipStream_t)stream, "dq_decode_wide_run");
        if (rc == DQ_ERR_RANGE) {                                  // a fused forward's own guard saw the same values: read and clear it, keep this message
            char msg[512];
            snprintf(msg, sizeof(msg), "%s", dq_last_error());
            (void)dq_qnet_range_check(net, stream);
            dq_set_error("%s", msg);
        }
        if (rc != DQ_OK) return rc;
    }
    if (iterations) *iterations = D->it;
    return dq_qnet_range_check(net, stream);                       // the fused forward's own guard, where it ran (dq_qnet_range_check[forward])
}

dq_status dq_decode_wide_rows(const dq_decode_wide* D, const uint8_t** rows_dev, int* row_bytes) {
    DQ_REQUIRE(D, DQ_ERR_INVALID, "dq_decode_wide_rows: null handle");
    if (rows_dev) *rows_dev = D->rows;
    if (row_bytes) *row_bytes = D->row_bytes;
    return DQ_OK;
}

dq_status dq_decode_wide_words(const dq_decode_wide* D, const uint64_t** legal_dev, const uint64_t** completed_dev, int* legal_words) {
    DQ_REQUIRE(D, DQ_ERR_INVALID, "dq_decode_wide_words: null handle");
    if (legal_dev) *legal_dev = D->legal;
    if (completed_dev) *completed_dev = D->comp;
    if (legal_words) *legal_words = D->LW;
    return DQ_OK;
}

dq_status dq_decode_wide_active(const dq_decode_wide* D, const int32_t** active_dev, int* n_active) {
    DQ_REQUIRE(D, DQ_ERR_INVALID, "dq_decode_wide_active: null handle");
    if (active_dev) *active_dev = D->act[D->cur];
    if (n_active) *n_active = D->n_active;
    return DQ_OK;
}

}  // extern "C"
