// work_carver.h -- the format of the d_work workspaces of the batch extension libraries (buffers.hip, buffers_decode.hip, frame_buffers.hip,
// layout.hip, frame_range.hip, frame_index.hip): typed pieces one after the other, each starting on a 256-byte boundary.  A layout function takes its pieces from one WorkCarver in a
// fixed order; with a null base (the sizing pass of the *_workspace functions) every piece is null and only bytes() counts.
#pragma once
#include "capi_internal.h"

struct WorkCarver {
    u8* base;
    u64 offset = 0;
    explicit WorkCarver(void* d_work) : base(static_cast<u8*>(d_work)) {}
    template <class T>
    T* take(u64 count)
    {
        T* const piece = base ? reinterpret_cast<T*>(base + offset) : nullptr;
        offset += snp_align_up(count * sizeof(T), 256);
        return piece;
    }
    u64 bytes() const { return offset; }
};
