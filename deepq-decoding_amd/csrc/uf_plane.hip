// The union-find referee as a stand-alone batched decode (include/deepq_hip.h dq_uf_referee_decode): uf_plane_dev.h's wave-level
// uf_plane_classify on given defects, one wavefront per syndrome, UFP_LDS bytes of dynamic LDS -- dq_match_decode's shape with the other referee.  The
// endpoint tables are the dq_wide_uf handle's.
#include "uf_plane_dev.h"
#include "uf_wide.h"

// one wave per syndrome: defects [batch][2 components][2 words], class = X part + 2 * Z part
__global__ __launch_bounds__(64) void uf_referee_decode_kernel(UfPlane ux, UfPlane uz, const u64* __restrict__ defects, int batch, int both, u8* __restrict__ cls) {
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= batch) return;                                         // wave-uniform
    const u64* dp = defects + (size_t)i * 4;
    const u64 x0 = dp[0], x1 = dp[1], z0 = dp[2], z1 = dp[3];       // (the same words in every lane: the compiler loads them as scalars)
    int c = uf_plane_classify(ux, x0, x1, smem, lane);
    if (both) c += 2 * uf_plane_classify(uz, z0, z1, smem, lane);
    if (lane == 0) cls[i] = (u8)c;
}

extern "C" {

dq_status dq_uf_referee_decode(const dq_wide_uf* H, const uint64_t* defects_dev, int batch, int both_components, uint8_t* class_dev, void* stream) {
    DQ_REQUIRE(H && defects_dev && class_dev, DQ_ERR_INVALID, "dq_uf_referee_decode: null argument");
    DQ_REQUIRE(batch >= 1, DQ_ERR_INVALID, "dq_uf_referee_decode: batch must be positive");
    const UfPlane ux = {H->ends, H->ends + 256, H->n, H->d, 0}, uz = {H->ends + 512, H->ends + 768, H->n, H->d, 1};
    uf_referee_decode_kernel<<<batch, 64, UFP_LDS, (hipStream_t)stream>>>(ux, uz, defects_dev, batch, both_components, class_dev);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

}  // extern "C"
