// frame_before_device.h -- before[b] = the largest clamped idx_first of the streams in front of stream b (0 for stream 0): what dd_stream
// (frame_dedup_device.h) takes to tell a stream that would share rows with an earlier one.  One kernel, shared by the calls that give every
// stream of a batch its verdict over all rows of the index: the dedup (frame_dedup.hip) and the verify (frame_verify.hip).
#pragma once
#include "frame_dedup_device.h"

namespace {

constexpr u32 kBeforeItems = 4;

// One workgroup: before[b] = the largest clamped idx_first[j], j < b.
__global__ __launch_bounds__(256) void k_fr_before(FrameIndex x, u32 ns, u64* __restrict__ before)
{
    __shared__ u64 s_wave[4];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    u64 carry = 0;
    for (u64 base = 0; base < ns; base += 256u * kBeforeItems) {
        const u64 i0 = base + static_cast<u64>(tid) * kBeforeItems;
        u64 v[kBeforeItems], m = 0;
        for (u32 k = 0; k < kBeforeItems; ++k) {
            v[k] = i0 + k < ns ? dd_first(x, i0 + k) : 0;
            m = v[k] > m ? v[k] : m;
        }
        u64 incl = m;                                                   // running maximum over the wavefront, this thread's items included
        for (u32 d = 1; d < 64; d <<= 1) {
            const u64 y = __shfl_up(incl, d, 64);
            if (lane >= d) incl = y > incl ? y : incl;
        }
        u64 excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0;
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        u64 run = carry, all = carry;
        for (u32 q = 0; q < 4; ++q) {
            if (q < wave) run = s_wave[q] > run ? s_wave[q] : run;
            all = s_wave[q] > all ? s_wave[q] : all;
        }
        __syncthreads();
        run = excl > run ? excl : run;
        for (u32 k = 0; k < kBeforeItems; ++k) {
            if (i0 + k < ns) before[i0 + k] = run;
            run = v[k] > run ? v[k] : run;
        }
        carry = all;
    }
}

}  // namespace
