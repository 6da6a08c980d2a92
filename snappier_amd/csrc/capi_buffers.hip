// capi_buffers.hip -- snp_compress_buffers_batch: many device buffers of ANY length, each compressed to ONE Snappy block
// (SnappyCompressor.TryCompress  SnappyCompressor.cs:24-83), entirely on the device.  The host-pointer snp_try_compress does the same job for one
// buffer with a read-back and a host prefix sum (capi_host.hip, compress_spans); here the plan, the scans and the emit are kernels (buffers.hip)
// around one launch of the existing compressor, nothing is read back, and the call can be captured like the other _batch entry points.
// Built into libsnappier_hip_buffers.so (C-ABI: include/snappier_hip_buffers.h), which is linked against libsnappier_hip.so and drives its
// contexts through the same snp_ctx members as capi_batch.hip.
#include "capi_internal.h"
#include "../../include/snappier_hip_buffers.h"

// d_work layout (every piece 256-byte aligned).  Per buffer: first fragment (nbuffers + 1, the last = fragments needed) and the tile sums of
// its scan; per fragment slot: input offset and length, staging offset, compressed length, status, owning buffer, the scan of the compressed
// lengths (max_fragments + 1) and its tile sums; then the staging area, kSnpCompStride bytes per slot (the compressor's output bound, padded).
struct BuffersWork {
    u64 *first, *first_part, *frag_in_off, *frag_stage_off, *frag_scan, *frag_part;
    u32 *frag_in_len, *frag_comp_len, *frag_owner;
    i32* frag_status;
    u8* stage;
    u64 bytes;
};
static BuffersWork buffers_work_layout(void* base, u32 nbuffers, u32 max_fragments)
{
    BuffersWork w{};
    if (nbuffers == 0) return w;                                         // (nothing is launched but the result)
    const u64 nb = nbuffers, nf = max_fragments;
    auto tiles = [](u64 n) { return (n + SNP_SCAN_TILE - 1) / SNP_SCAN_TILE + 1; };
    u8* p = static_cast<u8*>(base);
    u64 o = 0;
    auto take = [&](u64 bytes) { u8* r = p ? p + o : nullptr; o += snp_align_up(bytes, 256); return r; };
    w.first = reinterpret_cast<u64*>(take((nb + 1) * 8));
    w.first_part = reinterpret_cast<u64*>(take(tiles(nb) * 8));
    w.frag_scan = reinterpret_cast<u64*>(take((nf + 1) * 8));
    w.frag_part = reinterpret_cast<u64*>(take(tiles(nf) * 8));
    w.frag_in_off = reinterpret_cast<u64*>(take(nf * 8));
    w.frag_stage_off = reinterpret_cast<u64*>(take(nf * 8));
    w.frag_in_len = reinterpret_cast<u32*>(take(nf * 4));
    w.frag_comp_len = reinterpret_cast<u32*>(take(nf * 4));
    w.frag_owner = reinterpret_cast<u32*>(take(nf * 4));
    w.frag_status = reinterpret_cast<i32*>(take(nf * 4));
    w.stage = take(nf * kSnpCompStride);
    w.bytes = o;
    return w;
}

extern "C" {

uint64_t snp_compress_buffers_workspace(uint32_t nbuffers, uint32_t max_fragments)
{
    return buffers_work_layout(nullptr, nbuffers, max_fragments).bytes;
}

snp_status snp_compress_buffers_batch(snp_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nbuffers,
                                      uint32_t max_fragments, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                                      uint64_t* out_len, int32_t* status, void* d_work, uint64_t* d_result)
{
    if (!c || !d_result || (nbuffers && (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !status || !d_work)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    if (nbuffers == 0) return c->check(snp_launch_buffers_result_empty(d_result, s), "buffers result") ? SNP_OK : SNP_ERR_DEVICE;
    const BuffersWork w = buffers_work_layout(d_work, nbuffers, max_fragments);
    // plan: first fragment of every buffer (d_result[0] = fragments needed), then the fragment table over all max_fragments slots
    bool ok = c->check(snp_launch_buffers_first(in_len, nbuffers, w.first_part, w.first, d_result, s), "buffers scan") &&
              c->check(snp_launch_buffers_plan(in_off, in_len, nbuffers, w.first, max_fragments, kSnpCompStride, w.frag_in_off, w.frag_in_len,
                                               w.frag_stage_off, w.frag_owner, s), "buffers plan");
    // compress: every slot, the empty ones included (the count picks the layout: DESIGN.md 4.9), no varint -- CompressFragment only
    if (max_fragments)
        ok = ok && c->launch_compress(in, w.frag_in_off, w.frag_in_len, max_fragments, w.stage, w.frag_stage_off, w.frag_comp_len, w.frag_status, 0);
    // sizes, then the fragments to their places (a buffer that is not OK is not written at all)
    ok = ok && c->check(snp_launch_buffers_frag_scan(w.frag_comp_len, max_fragments, w.frag_part, w.frag_scan, s), "fragment scan") &&
         c->check(snp_launch_buffers_sizes(in_len, nbuffers, w.first, max_fragments, w.frag_scan, out, out_off, out_cap, out_len, status,
                                           d_result, s), "buffers sizes") &&
         c->check(snp_launch_buffers_emit(w.frag_owner, w.frag_comp_len, w.frag_scan, w.first, in_len, status, w.stage, kSnpCompStride, out,
                                          out_off, max_fragments, s), "buffers emit");
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

}  // extern "C"
