// The refereed verdict for any odd d in 3 .. 15 (include/deepq_hip.h dq_wide_uf_verdict_refereed): what the step decides on a hidden
// state (the reference's Environments.py:139-151) for the residual = hidden XOR frame, with the matching referee (match_dev.h) in the place
// of the look-up referee -- dq_decode_verdict's byte at the sizes where no table exists, env_big.hip's step rule without the step.
//   verdict_wide_refereed_kernel   one wavefront per volume, DQ_MATCH_LDS bytes of dynamic LDS (four volumes per CU, as match_decode_kernel).  The residual's
//                                  two planes are ballots of lane l's sites l, l + 64, ... (VW_WORDS words each, statically indexed); the defect words of each
//                                  component are ballots of node lane + 64 ww's parity, in the look-up referee's index order (lattice_host.h `typed`); a
//                                  residual in the code space leaves before the matching's LDS is touched (wave-uniform; the referee gives class 0 to the
//                                  empty syndrome, so decoded = 0 is exact)
// verdict_wide_refereed_kernel<true> (dq_wide_uf_verdict_refereed_uf) is the same kernel with the union-find referee (uf_plane_dev.h) in
// the matching's place: UFP_LDS bytes of dynamic LDS, no referee handle, no flags.  The flag is compile-time: the matching kernel carries no code of the other.
// verdict_wide_kernel (uf_wide.hip) stays the unrefereed form: in_code and cls here are its definitions bit for bit.
#include "match_dev.h"
#include "uf_plane_dev.h"
#include "uf_wide.h"

#define VW_WORDS 4                                               // ceil(15^2 / 64) words per plane

void match_comp(const struct dq_match* M, int comp, MatchComp* out);     // match.hip
dq_status match_reset_locks(const struct dq_match* M, hipStream_t st);   // match.hip: the scratch pool's lock words, in front of every launch that may take a slot

namespace {

struct VerdictRefArgs {
    MatchComp mx, mz;
    const u8 *node_stab;        // [2][128] node of component c -> stabilizer in measurement order, 255: no node
    const u8 *stab_q;           // [256][4] stabilizer -> its qubits, 255: none
    int n_streams, d, d2, model;
    const u8* hidden;           // [n][d2] codes 0..3
    const u8* frame;            // [n][d2] or NULL (no correction)
    u8* verdict;                // [n]
    u8* inexact;                // [n] or NULL
};

// bit q of the plane whose words are w[0 .. VW_WORDS): every index is a constant after unrolling
static __device__ __forceinline__ int plane_bit(const u64 (&w)[VW_WORDS], int q) {
    u64 word = 0;
#pragma unroll
    for (int k = 0; k < VW_WORDS; ++k) word = (q >> 6) == k ? w[k] : word;
    return (int)((word >> (q & 63)) & 1);
}

// The union-find launch takes the matching one's arguments with its two endpoint tables behind them.
struct VerdictRefArgsUf : VerdictRefArgs {
    UfPlane ux, uz;
};
template <bool Uf>
using VerdictRefArgsOf = std::conditional_t<Uf, VerdictRefArgsUf, VerdictRefArgs>;

template <bool Uf>
__global__ __launch_bounds__(64) void verdict_wide_refereed_kernel(VerdictRefArgsOf<Uf> p) {
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= p.n_streams) return;                                   // wave-uniform
    const u8* hid = p.hidden + (size_t)i * p.d2;
    const u8* frm = p.frame ? p.frame + (size_t)i * p.d2 : nullptr;
    // codes 1, 2 carry an X component, codes 2, 3 a Z component; the product of two Paulis is the XOR of the components
    u64 x[VW_WORDS], z[VW_WORDS];
    int px = 0, pz = 0;
#pragma unroll
    for (int w = 0; w < VW_WORDS; ++w) {
        const int site = lane + 64 * w;
        int h = 0, f = 0;
        if (site < p.d2) {
            h = hid[site] & 3;
            if (frm) f = frm[site] & 3;
        }
        const bool bx = (h == 1 || h == 2) != (f == 1 || f == 2), bz = (h >= 2) != (f >= 2);
        x[w] = __ballot(bx); z[w] = __ballot(bz);
        const int row = site / p.d, col = site - row * p.d;
        px += __popcll(__ballot(bx && col == 0));                   // X parity on column 0
        pz += __popcll(__ballot(bz && row == 0));                   // Z parity on row 0
    }
    const int cls = (px & 1) + 2 * (pz & 1);
    // the true syndrome of the residual as the defect words of each component: node lane + 64 ww of component c (0: type-3 plaquettes, the X plane)
    u64 df[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int ww = 0; ww < 2; ++ww) {
            const int s = p.node_stab[UFW_NODE_SLOTS * c + 64 * ww + lane];
            int par = 0;
            if (s < 255) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int q = p.stab_q[4 * s + k];
                    if (q < 255) par ^= c == 0 ? plane_bit(x, q) : plane_bit(z, q);
                }
            }
            df[c][ww] = __ballot(par & 1);
        }
    const bool in_code = (df[0][0] | df[0][1] | df[1][0] | df[1][1]) == 0;
    u8* out = p.verdict + i;
    u8* flag_out = p.inexact ? p.inexact + i : nullptr;
    if (in_code) {                                                  // wave-uniform: the referee's class of the empty syndrome is 0
        if (lane == 0) {
            *out = (u8)(DQ_VERDICT_IN_CODESPACE | (cls << DQ_VERDICT_CLASS_SHIFT) | (cls == 0 ? DQ_VERDICT_SUCCESS | DQ_VERDICT_ALIVE : 0));
            if (flag_out) *flag_out = 0;
        }
        return;
    }
    int flag = 0;
    int dec;
    if constexpr (Uf) {
        dec = uf_plane_classify(p.ux, df[0][0], df[0][1], smem, lane);
        if (p.model != DQ_MODEL_X) dec += 2 * uf_plane_classify(p.uz, df[1][0], df[1][1], smem, lane);
    } else {
        dec = match_classify(p.mx, df[0][0], df[0][1], smem, lane, &flag);
        if (p.model != DQ_MODEL_X) dec += 2 * match_classify(p.mz, df[1][0], df[1][1], smem, lane, &flag);
    }
    if (lane == 0) {
        *out = (u8)((cls << DQ_VERDICT_CLASS_SHIFT) | (dec == cls ? DQ_VERDICT_ALIVE : 0) | ((dec & 3) << DQ_VERDICT_DECODED_SHIFT));
        if (flag_out) *flag_out = (u8)flag;
    }
}

static void verdict_ref_args(const dq_wide_uf* H, const uint8_t* hidden_dev, const uint8_t* frame_dev, int n, uint8_t* verdict_dev, VerdictRefArgs* a) {
    a->node_stab = H->node_stab; a->stab_q = H->stab_q; a->n_streams = n; a->d = H->d; a->d2 = H->d2; a->model = H->model;
    a->hidden = hidden_dev; a->frame = frame_dev; a->verdict = verdict_dev;
}

}  // namespace

extern "C" {

dq_status dq_wide_uf_verdict_refereed_uf(dq_wide_uf* H, const uint8_t* hidden_dev, const uint8_t* frame_dev, int n, uint8_t* verdict_dev, void* stream) {
    DQ_REQUIRE(H && hidden_dev && verdict_dev, DQ_ERR_INVALID, "dq_wide_uf_verdict_refereed_uf: null argument");
    DQ_REQUIRE(n >= 1 && n <= H->max_streams, DQ_ERR_INVALID, "dq_wide_uf_verdict_refereed_uf: n = %d outside 1..max_streams %d", n, H->max_streams);
    VerdictRefArgsUf a;
    memset(&a, 0, sizeof(a));
    verdict_ref_args(H, hidden_dev, frame_dev, n, verdict_dev, &a);
    a.ux = UfPlane{H->ends, H->ends + 256, H->n, H->d, 0};
    a.uz = UfPlane{H->ends + 512, H->ends + 768, H->n, H->d, 1};
    verdict_wide_refereed_kernel<true><<<n, 64, UFP_LDS, (hipStream_t)stream>>>(a);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

dq_status dq_wide_uf_verdict_refereed(dq_wide_uf* H, const dq_match* M, const uint8_t* hidden_dev, const uint8_t* frame_dev, int n, uint8_t* verdict_dev,
                                      uint8_t* inexact_dev, void* stream) {
    DQ_REQUIRE(H && M && hidden_dev && verdict_dev, DQ_ERR_INVALID, "dq_wide_uf_verdict_refereed: null argument");
    DQ_REQUIRE(n >= 1 && n <= H->max_streams, DQ_ERR_INVALID, "dq_wide_uf_verdict_refereed: n = %d outside 1..max_streams %d", n, H->max_streams);
    int nodes = 0;
    { const dq_status rc = dq_match_info(M, &nodes, nullptr, nullptr); if (rc != DQ_OK) return rc; }
    DQ_REQUIRE(nodes == H->n, DQ_ERR_INVALID, "dq_wide_uf_verdict_refereed: the referee's lattice (%d nodes per component) is not the handle's (d = %d, %d nodes)",
               nodes, H->d, H->n);
    hipStream_t st = (hipStream_t)stream;
    static unsigned long long attr_devs = 0;                          // per device (common.h dq_device_bit)
    const unsigned long long dev_bit = dq_device_bit();
    if (!(attr_devs & dev_bit)) {
        const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void*>(verdict_wide_refereed_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, DQ_MATCH_LDS);
        if (ae != hipSuccess) {
            (void)hipGetLastError();
            dq_set_error("dq_wide_uf_verdict_refereed: hipFuncSetAttribute: %s", hipGetErrorString(ae));
            return DQ_ERR_HIP;
        }
        attr_devs |= dev_bit;
    }
    VerdictRefArgs a;
    memset(&a, 0, sizeof(a));
    match_comp(M, 0, &a.mx);
    match_comp(M, 1, &a.mz);
    verdict_ref_args(H, hidden_dev, frame_dev, n, verdict_dev, &a);
    a.inexact = inexact_dev;
    { const dq_status rc = match_reset_locks(M, st); if (rc != DQ_OK) return rc; }
    verdict_wide_refereed_kernel<false><<<n, 64, DQ_MATCH_LDS, st>>>(a);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

}  // extern "C"
