// Scoring batched decoding on the device (include/deepq_hip.h dq_decode_sample / dq_decode_verdict / dq_decode_count): the loop around dq_decode_run,
//   sample -> decode -> verdict -> counts,
// with nothing but the counters leaving the device.
//   eval_sample_kernel    n independent memory experiments from a clean lattice, one per wavefront: `depth` rounds of generate_error +
//                         generate_faulty_syndrome (the round of env_dev.h env_block's volume loop, ENV:157-170, WITHOUT the redraw of all-zero
//                         volumes, ENV:171) under the environment's Philox convention -- key = seed, lattice id = env_id_base + i, round counter
//                         0 .. depth - 1, lane = site --, so volume i is the first `depth` rounds of lattice env_id_base + i.  Out: the volumes in
//                         dq_decode_run's input layout, the accumulated error as hidden_state codes, one "all-zero volume" flag per volume.
//   eval_verdict_kernel   per volume, one per wavefront: residual = hidden XOR frame (obtain_new_error_configuration, FL:226-241), then what step()
//                         decides on that hidden state (ENV:139-151): perfect syndrome, homology class, the class the environment handle's
//                         installed referee assigns to the syndrome -- the arithmetic of env_block's step, the tables read through the handle.
//   eval_count_kernel     the flags summed into EVAL_COUNTERS 64-bit counters per contiguous block of volumes (one error rate per block).
#include "env_dev.h"

#define EVAL_THREADS 256         // sample / verdict: one volume per wavefront, four per workgroup
#define EVAL_COUNT_THREADS 1024  // count: one volume per thread
#define EVAL_COUNTERS DQ_EVAL_COUNTERS

namespace {

struct EvalSampleArgs {
    const EnvTables* tab;
    int n, d, d2, n_stab, depth, G, model;
    u32 env_id_base, seed0, seed1;
    u64 T_phys, T_meas;
    const u64* T_each;          // != NULL: [2 i] / [2 i + 1] = thresholds of volume i (common.h DqRateTable)
    u8* volumes;                // [n][depth][G]
    u8* hidden;                 // [n][d2]
    u8* trivial;                // [n]
};

__global__ __launch_bounds__(EVAL_THREADS) void eval_sample_kernel(EvalSampleArgs p) {
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (EVAL_THREADS / 64) + (threadIdx.x >> 6)));
    if (i >= p.n) return;                                           // wave-uniform
    const EnvTables* __restrict__ T = p.tab;
    const u64 sq = T->stab_qmask[lane];
    const bool isx = T->stab_isx[lane] != 0;
    // lane c < G owns cell (a, b) of the (d+1)^2 grid: the stabilizer padding_syndrome shows at the padded plane's cell (2a, 2b), none at a dead corner
    int sidx = 255;
    if (lane < p.G) {
        const int a = lane / (p.d + 1), b = lane - a * (p.d + 1);
        sidx = T->cell_stab[2 * a * (2 * p.d + 1) + 2 * b];
    }
    u64 T_phys = p.T_phys, T_meas = p.T_meas;
    if (p.T_each != nullptr) { T_phys = p.T_each[2 * (size_t)i]; T_meas = p.T_each[2 * (size_t)i + 1]; }
    u64 xmask = 0, zmask = 0, summed = 0;
    for (int j = 0; j < p.depth; ++j) {                              // env_block's round, round counter j
        u32 w[4];
        philox4x32_10((u32)j, 0u, p.env_id_base + (u32)i, (u32)lane, p.seed0, p.seed1, w);
        const bool hit = lane < p.d2 && (u64)w[0] < T_phys;         // FL:99 / FL:119
        const int typ = p.model == DQ_MODEL_X ? 1 : 1 + (int)__umulhi(w[1], 3u);   // FL:100
        const bool zhit = lane < p.d2 && (u64)w[1] < T_phys;        // IIDXZ (FL:134-160): the second uniform is an independent Z flip
        const u64 ex = __ballot(p.model == DQ_MODEL_IIDXZ ? hit : hit && typ != 3);
        const u64 ez = __ballot(p.model == DQ_MODEL_IIDXZ ? zhit : hit && typ != 1);
        const u64 flips = __ballot(lane < p.n_stab && (u64)w[2] < T_meas);         // FL:191-221
        xmask ^= ex;                                                // ENV:164, FL:226-241
        zmask ^= ez;
        const u64 tw = __ballot(__popcll((isx ? xmask : zmask) & sq) & 1);         // ENV:165
        const u64 v = tw ^ flips;                                   // ENV:166
        summed |= v;
        if (lane < p.G) p.volumes[((size_t)i * p.depth + j) * p.G + lane] = sidx < 64 ? (u8)((v >> sidx) & 1) : (u8)0;
    }
    if (lane < p.d2) {
        const int x = (int)((xmask >> lane) & 1), z = (int)((zmask >> lane) & 1);
        p.hidden[(size_t)i * p.d2 + lane] = (u8)(x ? (z ? 2 : 1) : (z ? 3 : 0));
    }
    if (lane == 0) p.trivial[i] = (u8)(summed == 0);
}

struct EvalVerdictArgs {
    const EnvTables* tab;
    const u32 *lut_x, *lut_z, *lut_joint;
    const u8* dec_in;           // != NULL: the Dense stack's class per volume (env.hip referee_mlp_kernel over xz_out of a first pass)
    int n, d2, model;
    const u8* hidden;           // [n][d2] codes 0..3
    const u8* frame;            // [n][d2] or NULL (no correction)
    u64* xz_out;                // != NULL: this pass only writes the residual's planes, [2 i] = X, [2 i + 1] = Z
    u8* verdict;                // [n]
};

__global__ __launch_bounds__(EVAL_THREADS) void eval_verdict_kernel(EvalVerdictArgs p) {
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (EVAL_THREADS / 64) + (threadIdx.x >> 6)));
    if (i >= p.n) return;                                           // wave-uniform
    const EnvTables* __restrict__ T = p.tab;
    const u64 sq = T->stab_qmask[lane];
    const bool isx = T->stab_isx[lane] != 0;
    const int rsrc = T->ref_src[lane];
    const u64 col0 = T->col0, row0 = T->row0;
    int h = 0, f = 0;
    if (lane < p.d2) {
        h = p.hidden[(size_t)i * p.d2 + lane] & 3;
        if (p.frame) f = p.frame[(size_t)i * p.d2 + lane] & 3;
    }
    // codes 1, 2 carry an X component, codes 2, 3 a Z component; the product of two Paulis is the XOR of the components (FL:54-62)
    const u64 xmask = __ballot(((h == 1 || h == 2) != (f == 1 || f == 2)));
    const u64 zmask = __ballot(((h >= 2) != (f >= 2)));
    if (p.xz_out) {
        if (lane == 0) { p.xz_out[2 * (size_t)i] = xmask; p.xz_out[2 * (size_t)i + 1] = zmask; }
        return;
    }
    const u64 true_word = __ballot(__popcll((isx ? xmask : zmask) & sq) & 1);       // ENV:139, FL:152-174
    const int cls = (__popcll(xmask & col0) & 1) + 2 * (__popcll(zmask & row0) & 1);    // ENV:143
    const u64 refw = __ballot(rsrc < 64 && ((true_word >> (rsrc & 63)) & 1));
    const u32 ix = (u32)refw, iz = (u32)(refw >> 32);
    int dec;
    if (p.dec_in) {
        dec = p.dec_in[i];
    } else if (p.lut_joint) {
        const u32 sw = (u32)true_word;
        dec = (p.lut_joint[sw >> 4] >> (2 * (sw & 15))) & 3;
    } else {
        dec = (p.lut_x[ix >> 5] >> (ix & 31)) & 1;                  // ENV:144
        if (p.model != DQ_MODEL_X) dec += 2 * ((p.lut_z[iz >> 5] >> (iz & 31)) & 1);
    }
    const bool in_code = true_word == 0;
    const bool success = cls == 0 && in_code;                       // ENV:148-149: the step's reward 1
    const bool alive = success || dec == cls;                       // ENV:150-151: the step's done == False
    if (lane == 0)
        p.verdict[i] = (u8)((in_code ? DQ_VERDICT_IN_CODESPACE : 0) | (cls << DQ_VERDICT_CLASS_SHIFT) | (success ? DQ_VERDICT_SUCCESS : 0) |
                            (alive ? DQ_VERDICT_ALIVE : 0) | ((dec & 3) << DQ_VERDICT_DECODED_SHIFT));
}

struct EvalCountArgs {
    const u8* verdict;
    const u8* trivial;          // or NULL
    const u8* status;           // or NULL
    const int32_t* n_corr;      // or NULL
    int n, block;
    long long first;            // global index of volume 0: volume i counts into block (first + i) / block
    unsigned long long* counters;
};

// A workgroup's volumes mostly lie in one block: those are summed in LDS and leave as EVAL_COUNTERS atomics per workgroup; a wave of another block adds
// its ballots' counts itself, a wave that straddles two blocks adds per thread.  Integer sums: order-independent.
__global__ __launch_bounds__(EVAL_COUNT_THREADS) void eval_count_kernel(EvalCountArgs p) {
    __shared__ unsigned long long s_c[EVAL_COUNTERS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = blockIdx.x * EVAL_COUNT_THREADS + tid;
    const bool in = i < p.n;
    const long long wg_bid = (p.first + (long long)blockIdx.x * EVAL_COUNT_THREADS) / p.block;
    const long long bid = in ? (p.first + i) / p.block : -1;
    if (tid < EVAL_COUNTERS) s_c[tid] = 0;
    __syncthreads();
    const int v = in ? p.verdict[i] : 0;
    const int st = in && p.status ? p.status[i] : 0;
    unsigned long long val[EVAL_COUNTERS];
    val[DQ_EVAL_VOLUMES] = in;
    val[DQ_EVAL_TRIVIAL] = in && p.trivial && p.trivial[i];
    val[DQ_EVAL_IN_CODESPACE] = (v & DQ_VERDICT_IN_CODESPACE) != 0;
    val[DQ_EVAL_SUCCESS] = (v & DQ_VERDICT_SUCCESS) != 0;
    val[DQ_EVAL_ALIVE] = (v & DQ_VERDICT_ALIVE) != 0;
    val[DQ_EVAL_IDENTITY] = st == DQ_DECODE_IDENTITY;
    val[DQ_EVAL_REPEAT] = st == DQ_DECODE_REPEAT;
    val[DQ_EVAL_STOPPED] = st == DQ_DECODE_STOPPED;
    val[DQ_EVAL_CORRECTIONS] = in && p.n_corr ? (unsigned long long)p.n_corr[i] : 0ull;
    const long long b0 = __shfl(bid, 0);                            // (`in` is a prefix of the wave: lane 0 out of range <=> the whole wave is)
    if (__all(!in || bid == b0)) {
        if (b0 >= 0) {
#pragma unroll
            for (int k = 0; k < EVAL_COUNTERS; ++k) {
                unsigned long long c;
                if (k == DQ_EVAL_CORRECTIONS) {
                    c = val[k];
                    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
                } else {
                    c = (unsigned long long)__popcll(__ballot(val[k] != 0));
                }
                if (lane == 0 && c) atomicAdd(b0 == wg_bid ? &s_c[k] : &p.counters[b0 * EVAL_COUNTERS + k], c);
            }
        }
    } else if (in) {
#pragma unroll
        for (int k = 0; k < EVAL_COUNTERS; ++k)
            if (val[k]) atomicAdd(&p.counters[bid * EVAL_COUNTERS + k], val[k]);
    }
    __syncthreads();
    if (tid < EVAL_COUNTERS && s_c[tid]) atomicAdd(&p.counters[wg_bid * EVAL_COUNTERS + tid], s_c[tid]);
}

}  // namespace

#include "decode_eval.h"

static dq_status eval_same_lattice(const dq_decode_eval* V, const EnvRefereeView& R, bool depth_too, const char* who) {
    DQ_REQUIRE(R.d == V->d && R.model == V->model && (R.model == DQ_MODEL_X || (R.use_Y != 0) == (V->use_Y != 0)) && (!depth_too || R.depth == V->depth),
               DQ_ERR_INVALID, "%s: the environment's lattice (d = %d, model %d, use_Y = %d, volume_depth = %d) is not the decoder's (d = %d, model %d, "
               "use_Y = %d, volume_depth = %d)", who, R.d, R.model, R.use_Y, R.depth, V->d, V->model, V->use_Y, V->depth);
    return DQ_OK;
}

extern "C" {

dq_status dq_decode_eval_create(const dq_decode_cfg* cfg, int max_volumes, dq_decode_eval** out) {
    DQ_REQUIRE(cfg && out, DQ_ERR_INVALID, "dq_decode_eval_create: null argument");
    *out = nullptr;
    DQ_REQUIRE(cfg->d >= 3 && (cfg->d & 1), DQ_ERR_INVALID, "dq_decode_eval_create: d must be odd and >= 3");
    DQ_REQUIRE(cfg->d <= 7, DQ_ERR_UNSUPPORTED, "dq_decode_eval_create: d = %d: decoding covers the one-wavefront lattices, d <= 7", cfg->d);
    DQ_REQUIRE(cfg->volume_depth >= 1 && cfg->volume_depth <= 16, DQ_ERR_INVALID, "dq_decode_eval_create: volume_depth must be in 1..16");
    DQ_REQUIRE(cfg->error_model >= DQ_MODEL_X && cfg->error_model <= DQ_MODEL_IIDXZ, DQ_ERR_INVALID, "dq_decode_eval_create: bad error model");
    const int layers = cfg->error_model == DQ_MODEL_X ? 1 : (cfg->use_Y ? 3 : 2);
    DQ_REQUIRE(layers * cfg->d * cfg->d + 1 <= 128, DQ_ERR_UNSUPPORTED, "dq_decode_eval_create: %d actions: decoding holds 128", layers * cfg->d * cfg->d + 1);
    DQ_REQUIRE(max_volumes >= 1, DQ_ERR_INVALID, "dq_decode_eval_create: max_volumes must be >= 1");
    dq_decode_eval* V = new dq_decode_eval();
    memset(V, 0, sizeof(*V));
    V->d = cfg->d; V->depth = cfg->volume_depth; V->model = cfg->error_model; V->use_Y = cfg->use_Y ? 1 : 0; V->max_volumes = max_volumes;
    const size_t bytes = (2 * (size_t)max_volumes + 2) * sizeof(u64);
    hipError_t e = hipMalloc(&V->rates.dev, bytes);
    if (e == hipSuccess) e = hipHostMalloc(&V->rates.host, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&V->rates.copied, hipEventDisableTiming);
    if (e != hipSuccess) {
        dq_set_error("dq_decode_eval_create: %s", hipGetErrorString(e));
        dq_decode_eval_destroy(V);
        return e == hipErrorOutOfMemory ? DQ_ERR_NOMEM : DQ_ERR_HIP;
    }
    *out = V;
    return DQ_OK;
}

void dq_decode_eval_destroy(dq_decode_eval* V) {
    if (!V) return;
    dq_rate_table_free(V->rates);
    if (V->xz) (void)hipFree(V->xz);
    if (V->no_action) (void)hipFree(V->no_action);
    if (V->dec) (void)hipFree(V->dec);
    match_st_free(V->match_st);
    delete V;
}

dq_status dq_decode_sample(dq_decode_eval* V, const dq_env* env, int n, uint32_t env_id_base, const uint32_t seed[2], double p_phys, double p_meas,
                           const double* p_phys_each, const double* p_meas_each, uint8_t* volumes_dev, uint8_t* hidden_dev, uint8_t* trivial_dev,
                           void* stream) {
    DQ_REQUIRE(V && env && seed && volumes_dev && hidden_dev && trivial_dev, DQ_ERR_INVALID, "dq_decode_sample: null argument");
    DQ_REQUIRE(n >= 1 && n <= V->max_volumes, DQ_ERR_INVALID, "dq_decode_sample: n = %d outside 1..max_volumes %d", n, V->max_volumes);
    DQ_REQUIRE((reinterpret_cast<uintptr_t>(volumes_dev) & 3) == 0, DQ_ERR_INVALID, "dq_decode_sample: volumes_dev must be 4-byte aligned (dq_decode_run reads it)");
    DQ_REQUIRE((p_phys_each != nullptr) == (p_meas_each != nullptr), DQ_ERR_INVALID, "dq_decode_sample: per-volume rates come as a pair of arrays");
    EnvRefereeView R;
    dq_status rc = env_referee_view(env, false, &R);
    if (rc != DQ_OK) return rc;
    rc = eval_same_lattice(V, R, true, "dq_decode_sample");
    if (rc != DQ_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    EvalSampleArgs a;
    memset(&a, 0, sizeof(a));
    if (p_phys_each) {
        rc = dq_rate_table_upload(V->rates, n, p_phys_each, p_meas_each, st);
        if (rc != DQ_OK) return rc;
        a.T_each = V->rates.dev;
    } else {
        DQ_REQUIRE(p_phys >= 0.0 && p_phys <= 1.0 && p_meas >= 0.0 && p_meas <= 1.0, DQ_ERR_INVALID, "dq_decode_sample: rates must be in [0,1]");
        a.T_phys = dq_rate_threshold(p_phys); a.T_meas = dq_rate_threshold(p_meas);
    }
    a.tab = R.tab; a.n = n; a.d = R.d; a.d2 = R.d * R.d; a.n_stab = R.n_stab; a.depth = V->depth; a.G = (R.d + 1) * (R.d + 1); a.model = R.model;
    a.env_id_base = env_id_base; a.seed0 = seed[0]; a.seed1 = seed[1];
    a.volumes = volumes_dev; a.hidden = hidden_dev; a.trivial = trivial_dev;
    const int wpb = EVAL_THREADS / 64;
    eval_sample_kernel<<<(n + wpb - 1) / wpb, EVAL_THREADS, 0, st>>>(a);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

dq_status dq_decode_verdict(dq_decode_eval* V, dq_env* env, const uint8_t* hidden_dev, const uint8_t* frame_dev, int n, uint8_t* verdict_dev, void* stream) {
    DQ_REQUIRE(V && env && hidden_dev && verdict_dev, DQ_ERR_INVALID, "dq_decode_verdict: null argument");
    DQ_REQUIRE(n >= 1 && n <= V->max_volumes, DQ_ERR_INVALID, "dq_decode_verdict: n = %d outside 1..max_volumes %d", n, V->max_volumes);
    EnvRefereeView R;
    dq_status rc = env_referee_view(env, true, &R);
    if (rc != DQ_OK) return rc;
    rc = eval_same_lattice(V, R, false, "dq_decode_verdict");
    if (rc != DQ_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    EvalVerdictArgs a;
    memset(&a, 0, sizeof(a));
    a.tab = R.tab; a.lut_x = R.lut_x; a.lut_z = R.lut_z; a.lut_joint = R.lut_joint; a.n = n; a.d2 = R.d * R.d; a.model = R.model;
    a.hidden = hidden_dev; a.frame = frame_dev; a.verdict = verdict_dev;
    const int wpb = EVAL_THREADS / 64, blocks = (n + wpb - 1) / wpb;
    if (R.mlp) {                                                    // the Dense stack: residual planes out, the stack's classes, then the verdict
        if (!V->xz) {
            const size_t words = 2 * (size_t)V->max_volumes + 16;
            DQ_HIP(hipMalloc(&V->xz, words * sizeof(u64)));
            DQ_HIP(hipMemset(V->xz, 0, words * sizeof(u64)));
            DQ_HIP(hipMalloc(&V->no_action, (size_t)V->max_volumes * sizeof(int32_t)));
            DQ_HIP(hipMemset(V->no_action, 0xff, (size_t)V->max_volumes * sizeof(int32_t)));      // -1: outside the action range = no move
            DQ_HIP(hipMalloc(&V->dec, (size_t)V->max_volumes));
        }
        EvalVerdictArgs a0 = a;
        a0.xz_out = V->xz;
        eval_verdict_kernel<<<blocks, EVAL_THREADS, 0, st>>>(a0);
        DQ_LAUNCH_CHECK();
        rc = env_referee_mlp_classes(env, V->xz, 2, n, V->no_action, V->dec, st);
        if (rc != DQ_OK) return rc;
        a.dec_in = V->dec;
    }
    eval_verdict_kernel<<<blocks, EVAL_THREADS, 0, st>>>(a);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

dq_status dq_decode_count(const uint8_t* verdict_dev, const uint8_t* trivial_dev, const uint8_t* status_dev, const int32_t* n_corr_dev, int n,
                          int64_t first, int block, int n_blocks, uint64_t* counters_dev, void* stream) {
    DQ_REQUIRE(verdict_dev && counters_dev, DQ_ERR_INVALID, "dq_decode_count: null argument");
    DQ_REQUIRE(n >= 1 && block >= 1 && n_blocks >= 1 && first >= 0, DQ_ERR_INVALID, "dq_decode_count: n, block and n_blocks must be >= 1, first >= 0");
    DQ_REQUIRE((first + n - 1) / block < n_blocks, DQ_ERR_INVALID, "dq_decode_count: volumes %lld .. %lld in blocks of %d do not fit %d blocks of counters",
               (long long)first, (long long)first + n - 1, block, n_blocks);
    DQ_REQUIRE((reinterpret_cast<uintptr_t>(counters_dev) & 7) == 0 && (!n_corr_dev || (reinterpret_cast<uintptr_t>(n_corr_dev) & 3) == 0), DQ_ERR_INVALID,
               "dq_decode_count: counters_dev must be 8-byte, n_corr_dev 4-byte aligned");
    EvalCountArgs a;
    a.verdict = verdict_dev; a.trivial = trivial_dev; a.status = status_dev; a.n_corr = n_corr_dev; a.n = n; a.block = block; a.first = first;
    a.counters = reinterpret_cast<unsigned long long*>(counters_dev);
    eval_count_kernel<<<(n + EVAL_COUNT_THREADS - 1) / EVAL_COUNT_THREADS, EVAL_COUNT_THREADS, 0, (hipStream_t)stream>>>(a);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

}  // extern "C"
