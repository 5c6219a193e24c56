// The stable compaction of a decode's active list, shared by decode.hip and decode_wide.hip: partition b = positions [b DEC_PART, (b + 1) DEC_PART) of
// the list, one per thread of a workgroup of DEC_PART threads.  A partition's offset is the sum of the counts of the partitions before it (the selection
// launch adds them up), its volumes keep their order inside it; the last partition writes the active count.
#pragma once
#include "common.h"

#define DEC_PART 1024            // compaction partition: positions of the active list per compact workgroup (one per thread)

__device__ __forceinline__ void decode_compact_partition(const int* part, int* part_next, const int32_t* act_in, int n_active, const u8* status,
                                                         int32_t* act_out, int* count) {
    __shared__ int s_pre[DEC_PART / 64];
    __shared__ int s_cnt[DEC_PART / 64];
    __shared__ int s_base[DEC_PART / 64];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int pre = 0;                                                    // volumes of the partitions before this one that go on
    for (int k = t; k < b; k += DEC_PART) pre += part[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) pre += __shfl_xor(pre, m);
    const int pos = b * DEC_PART + t;
    const int v = pos < n_active ? act_in[pos] : 0;
    const bool keep = pos < n_active && status[v] == DQ_DECODE_ACTIVE;
    const u64 bal = __ballot(keep);
    if (lane == 0) { s_pre[wave] = pre; s_cnt[wave] = __popcll(bal); }
    __syncthreads();
    if (t == 0) {
        int off = 0;
        for (int w = 0; w < DEC_PART / 64; ++w) off += s_pre[w];
        for (int w = 0; w < DEC_PART / 64; ++w) { s_base[w] = off; off += s_cnt[w]; }
        if (b == (int)gridDim.x - 1) *count = off;
        part_next[b] = 0;                                           // the next iteration's counts start from zero
    }
    __syncthreads();
    if (keep) act_out[s_base[wave] + __popcll(bal & ((1ull << lane) - 1ull))] = v;
}
