// capi_frame.hip -- the framing format end to end (SnappyStreamCompressor.cs:18-21,166-261; SnappyStreamDecompressor.cs:38-208): orchestration of
// compress + masked CRC + raw-vs-compressed decision + scan + emit on the way in, header walk + decode + CRC verify on the way out.  The kernels are in
// framing.hip, frame_scan.hip, crc32c.hip and the codec files; this file only sequences them and moves host buffers.  The host walk over a stream's
// chunk headers (scan_chunks) is a loop over frame_hop (frame_hop_device.h), the hop the device walks take.
#include "capi_internal.h"
#include "frame_hop_device.h"

// workspace layout for snp_frame_encode_device (all sub-arrays 16-byte aligned)
struct FrameWork {
    u64 *in_off, *comp_off, *dst_off, *total;
    u32 *in_len, *comp_len, *payload, *crc;
    i32* status;
    u8 *type, *comp;
    u64 bytes;
};
static FrameWork frame_work_layout(void* base, u64 n)
{
    const u64 nc = (n + SNP_BLOCK_SIZE - 1) / SNP_BLOCK_SIZE;
    u8* p = static_cast<u8*>(base);
    u64 o = 0;
    FrameWork w{};
    auto take = [&](u64 bytes) { u8* r = p ? p + o : nullptr; o += snp_align_up(bytes, 16); return r; };
    w.in_off = reinterpret_cast<u64*>(take(nc * 8));
    w.comp_off = reinterpret_cast<u64*>(take(nc * 8));
    w.dst_off = reinterpret_cast<u64*>(take((nc + 1) * 8));
    w.total = reinterpret_cast<u64*>(take(8));
    w.in_len = reinterpret_cast<u32*>(take(nc * 4));
    w.comp_len = reinterpret_cast<u32*>(take(nc * 4));
    w.payload = reinterpret_cast<u32*>(take(nc * 4));
    w.crc = reinterpret_cast<u32*>(take(nc * 4));
    w.status = reinterpret_cast<i32*>(take(nc * 4));
    w.type = take(nc);
    w.comp = take(nc * kSnpCompStride);
    w.bytes = o;
    return w;
}


// host_in != nullptr: the raw stream is still in host memory; it is uploaded into d_in in slices that overlap the compressor
snp_status snp_frame_encode_impl(snp_ctx* c, const uint8_t* d_in, const uint8_t* host_in, uint64_t n, uint8_t* d_out,
                                    uint64_t cap, uint64_t* d_written, void* d_work)
{
    if (cap < SNP_STREAM_HEADER_LEN) return SNP_ERR_OUTPUT_TOO_SMALL;
    const u32 nc = static_cast<u32>((n + SNP_BLOCK_SIZE - 1) / SNP_BLOCK_SIZE);
    hipStream_t s = c->stream;
    if (nc == 0)
        return c->check(snp_launch_frame_header_only(d_out, d_written, s), "frame header") ? SNP_OK : SNP_ERR_DEVICE;
    const FrameWork w = frame_work_layout(d_work, n);
    bool ok = c->check(snp_launch_frame_chunks(n, nc, kSnpCompStride, w.in_off, w.in_len, w.comp_off, s), "frame chunks");
    // CompressBlock: TryCompress(chunk) = varint + one fragment  (SnappyStreamCompressor.cs:206)
    if (host_in) ok = ok && c->upload_and_compress(host_in, n, nc, w.in_off, w.in_len, w.comp, w.comp_off, w.comp_len, w.status, 1);
    else ok = ok && c->launch_compress(d_in, w.in_off, w.in_len, nc, w.comp, w.comp_off, w.comp_len, w.status, 1);
    // masked CRC-32C of the RAW chunk  (:243-245,258-260)
    ok = ok && c->check(snp_launch_crc32c(d_in, w.in_off, w.in_len, nc, 1 | c->crc_bits(), w.crc, nullptr, nullptr, s), "frame crc");
    ok = ok && c->check(snp_launch_frame_plan(w.in_len, w.comp_len, nc, w.type, w.payload, w.dst_off, d_written, s),
                        "frame plan");
    ok = ok && c->check(snp_launch_frame_emit(d_in, w.in_off, w.comp, w.comp_off, w.type, w.payload, w.crc, w.dst_off,
                                              d_out, cap, nc, s), "frame emit");
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

bool snp_ctx::decode_chunks(const u8* d_in, const ChunkRows& r, u32 n, u8* d_out)
{
    return launch_decompress(d_in, r.body_off, r.body_len, n, d_out, r.out_off, r.out_cap, r.out_len, r.status, r.type) &&
           check(snp_launch_crc32c(d_out, r.out_off, r.out_len, n, 1 | crc_bits(), nullptr, r.crc, r.status, stream), "frame crc verify");
}

// The chunk table of the one-stream calls, packed (no padding between the arrays; the order keeps every array aligned when base is 8-byte
// aligned): body_off, out_off (u64) ; body_len, crc, out_cap, out_len (u32) ; status (i32) ; type (u8).  snp_frame_decode_workspace promises
// this size, so the table is not carved by WorkCarver like those of the batch calls.
struct PackedRows {
    ChunkRows r;
    u64 bytes;
};
static PackedRows packed_chunk_rows(void* base, u64 n)
{
    u8* p = static_cast<u8*>(base);
    PackedRows w{};
    auto take = [&](u64 bytes) { u8* piece = p ? p + w.bytes : nullptr; w.bytes += bytes; return piece; };
    w.r.body_off = reinterpret_cast<u64*>(take(n * 8));
    w.r.out_off = reinterpret_cast<u64*>(take(n * 8));
    w.r.body_len = reinterpret_cast<u32*>(take(n * 4));
    w.r.crc = reinterpret_cast<u32*>(take(n * 4));
    w.r.out_cap = reinterpret_cast<u32*>(take(n * 4));
    w.r.out_len = reinterpret_cast<u32*>(take(n * 4));
    w.r.status = reinterpret_cast<i32*>(take(n * 4));
    w.r.type = take(n);
    return w;
}

extern "C" {

uint64_t snp_frame_encode_workspace(uint64_t n) { return frame_work_layout(nullptr, n).bytes; }

snp_status snp_frame_encode_device(snp_ctx* c, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap,
                                   uint64_t* d_written, void* d_work)
{
    if (!c || !d_out || !d_written || !d_work || (n && !d_in)) return SNP_ERR_BAD_ARG;
    if (n > 0xffffffffull * SNP_BLOCK_SIZE) return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    return snp_frame_encode_impl(c, d_in, nullptr, n, d_out, cap, d_written, d_work);
}

snp_status snp_frame_decode_chunks_device(snp_ctx* c, const uint8_t* d_in, const uint8_t* chunk_type,
                                          const uint64_t* body_off, const uint32_t* body_len,
                                          const uint32_t* chunk_crc, uint32_t nchunks, uint8_t* d_out,
                                          const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len,
                                          int32_t* status)
{
    if (!c || (nchunks && (!d_in || !chunk_type || !body_off || !body_len || !chunk_crc || !d_out || !out_off ||
                           !out_cap || !out_len || !status)))
        return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    ChunkRows r{};                                                      // (the caller's table: decode_chunks writes out_len and status only)
    r.type = const_cast<u8*>(chunk_type);
    r.body_off = const_cast<u64*>(body_off);
    r.body_len = const_cast<u32*>(body_len);
    r.crc = const_cast<u32*>(chunk_crc);
    r.out_off = const_cast<u64*>(out_off);
    r.out_cap = const_cast<u32*>(out_cap);
    r.out_len = out_len;
    r.status = status;
    return c->decode_chunks(d_in, r, nchunks, d_out) ? SNP_OK : SNP_ERR_DEVICE;
}

// ---- framed stream without a chunk table: header walk on the device --------------------------------
// workspace: 64-byte header {total, tail status, chunks} ; the packed chunk table ; 16 bytes
uint64_t snp_frame_decode_workspace(uint32_t max_chunks)
{
    return 64 + snp_align_up(packed_chunk_rows(nullptr, max_chunks).bytes, 16) + 16;
}

snp_status snp_frame_decode_device(snp_ctx* c, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap,
                                   uint32_t max_chunks, void* d_work, uint64_t* d_result)
{
    if (!c || !d_work || !d_result || (n && !d_in) || (cap && !d_out)) return SNP_ERR_BAD_ARG;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    u64* hdr = static_cast<u64*>(d_work);
    const ChunkRows r = packed_chunk_rows(hdr + 8, max_chunks).r;
    bool ok;
    if (c->frame_scan == 1) {
        ok = c->check(snp_launch_frame_scan(d_in, n, cap, max_chunks, r, hdr, s), "frame scan");
    } else {
        // per-span candidate tables live in context scratch (a few MB per 10 GiB of stream; grows on first use only)
        if (!c->ensure(c->scan, snp_frame_scan_workspace(n), "hipMalloc(frame scan)")) return SNP_ERR_DEVICE;
        ok = c->check(snp_launch_frame_scan_spans(d_in, n, cap, max_chunks, r, hdr, c->scan.p, s), "frame scan (spans)");
    }
    if (ok && max_chunks && n) {                     // n == 0: no chunk, nothing to launch
        if (!d_out) return SNP_ERR_BAD_ARG;          // (as snp_frame_decode_chunks_device: a table to decode needs an output, whatever cap is)
        if (!c->decode_chunks(d_in, r, max_chunks, d_out)) return SNP_ERR_DEVICE;
    }
    ok = ok && c->check(snp_launch_frame_result(r.status, hdr, d_result, s), "frame result");
    return ok ? SNP_OK : SNP_ERR_DEVICE;
}

snp_status snp_frame_encode(snp_ctx* c, const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* written)
{
    if (!c || !written || (n && !in) || (cap && !out)) return SNP_ERR_BAD_ARG;
    *written = 0;
    if (snp_ranges_overlap(in, n, out, cap)) return SNP_ERR_OVERLAP;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    hipStream_t s = c->stream;
    const u64 max_out = static_cast<u64>(snp_frame_max_encoded_length(static_cast<int64_t>(n)));
    const u64 wbytes = snp_frame_encode_workspace(n);
    if (!c->ensure(c->in, n + 16, "hipMalloc(in)") || !c->ensure(c->out, max_out + 16, "hipMalloc(out)") ||
        !c->ensure(c->work, wbytes + 16, "hipMalloc(work)") || !c->ensure(c->meta, 64, "hipMalloc(meta)"))
        return SNP_ERR_DEVICE;
    bool ok = true;
    if (n > 0xffffffffull * SNP_BLOCK_SIZE) return SNP_ERR_BAD_ARG;
    snp_status st = snp_frame_encode_impl(c, static_cast<const u8*>(c->in.p), n ? in : nullptr, n, static_cast<u8*>(c->out.p), max_out,
                                      static_cast<u64*>(c->meta.p), c->work.p);
    if (st != SNP_OK) return st;
    u64 total = 0;
    ok = c->check(hipMemcpyAsync(&total, c->meta.p, 8, hipMemcpyDeviceToHost, s), "D2H total") &&
         c->check(hipStreamSynchronize(s), "sync");
    if (!ok) return SNP_ERR_DEVICE;
    if (total > cap) return SNP_ERR_OUTPUT_TOO_SMALL;
    ok = c->d2h(out, c->out.p, total, "D2H output") &&
         c->check(hipStreamSynchronize(s), "sync");
    if (!ok) return SNP_ERR_DEVICE;
    *written = total;
    return SNP_OK;
}

// Host-side walk over chunk headers only (SnappyStreamDecompressor.ReadChunkHeader  :215-254): 4 bytes per chunk.
struct ChunkScan {
    std::vector<u8> type;
    std::vector<u64> body_off, out_off;
    std::vector<u32> body_len, crc, out_cap;
    u64 total = 0;
    snp_status tail = SNP_OK;   // error met after the chunks listed above (they are still decoded and checked first)
};
static void scan_chunks(const u8* in, size_t n, ChunkScan& cs)
{
    for (u64 ip = 0;;) {
        const Hop h = frame_hop(in, n, ip);
        if (h.kind == HOP_END) return;
        if (h.kind == HOP_ERR) { cs.tail = static_cast<snp_status>(h.err); return; }
        if (h.kind == HOP_DATA) {
            cs.type.push_back(static_cast<u8>(h.type));
            cs.body_off.push_back(ip + SNP_CHUNK_HEADER_LEN);
            cs.body_len.push_back(h.body_len);
            cs.crc.push_back(h.crc);
            cs.out_off.push_back(cs.total);
            cs.out_cap.push_back(h.dec);
            cs.total += h.dec;
        }
        ip = h.next;
    }
}

snp_status snp_frame_decoded_length(const uint8_t* in, size_t n, uint64_t* out_len)
{
    if (!out_len || (n && !in)) return SNP_ERR_BAD_ARG;
    ChunkScan cs;
    scan_chunks(in, n, cs);
    *out_len = cs.total;
    return cs.tail;
}

snp_status snp_frame_decode(snp_ctx* c, const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* written)
{
    if (!c || !written || (n && !in) || (cap && !out)) return SNP_ERR_BAD_ARG;
    *written = 0;
    DevGuard dg(c);
    if (!dg.ok) return SNP_ERR_DEVICE;
    ChunkScan cs;
    scan_chunks(in, n, cs);
    const u32 nc = static_cast<u32>(cs.type.size());
    if (cs.total > cap) return SNP_ERR_OUTPUT_TOO_SMALL;
    if (nc == 0) return cs.tail;
    hipStream_t s = c->stream;
    if (!c->ensure(c->in, n + 16, "hipMalloc(in)") || !c->ensure(c->out, cs.total + 16, "hipMalloc(out)") ||
        !c->ensure(c->meta, packed_chunk_rows(nullptr, nc).bytes + 64, "hipMalloc(meta)"))
        return SNP_ERR_DEVICE;
    const ChunkRows r = packed_chunk_rows(c->meta.p, nc).r;
    bool ok = c->h2d(c->in.p, in, n, "H2D input");
    ok = ok && c->check(hipMemcpyAsync(r.body_off, cs.body_off.data(), nc * 8ull, hipMemcpyHostToDevice, s), "H2D meta");
    ok = ok && c->check(hipMemcpyAsync(r.out_off, cs.out_off.data(), nc * 8ull, hipMemcpyHostToDevice, s), "H2D meta");
    ok = ok && c->check(hipMemcpyAsync(r.body_len, cs.body_len.data(), nc * 4ull, hipMemcpyHostToDevice, s), "H2D meta");
    ok = ok && c->check(hipMemcpyAsync(r.crc, cs.crc.data(), nc * 4ull, hipMemcpyHostToDevice, s), "H2D meta");
    ok = ok && c->check(hipMemcpyAsync(r.out_cap, cs.out_cap.data(), nc * 4ull, hipMemcpyHostToDevice, s), "H2D meta");
    ok = ok && c->check(hipMemcpyAsync(r.type, cs.type.data(), nc, hipMemcpyHostToDevice, s), "H2D meta");
    if (!ok || !c->decode_chunks(static_cast<const u8*>(c->in.p), r, nc, static_cast<u8*>(c->out.p))) return SNP_ERR_DEVICE;
    std::vector<i32> status(nc);
    ok = c->check(hipMemcpyAsync(status.data(), r.status, nc * 4ull, hipMemcpyDeviceToHost, s), "D2H status") &&
         c->check(hipStreamSynchronize(s), "sync");
    if (!ok) return SNP_ERR_DEVICE;
    for (u32 i = 0; i < nc; ++i)                                          // first failing chunk in stream order wins,
        if (status[i] != SNP_OK) return static_cast<snp_status>(status[i]);   // as the sequential reference would throw
    if (cs.tail != SNP_OK) return cs.tail;
    if (cs.total) {
        ok = c->d2h(out, c->out.p, cs.total, "D2H output") &&
             c->check(hipStreamSynchronize(s), "sync");
        if (!ok) return SNP_ERR_DEVICE;
    }
    *written = cs.total;
    return SNP_OK;
}

}  // extern "C"
