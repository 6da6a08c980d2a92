// tag_index.hip -- finds where the 64 KiB output fragments of ONE large Snappy block begin in its compressed stream,
// so that the block can be decoded by one wavefront per fragment instead of one wavefront for the whole block
// (SnappyDecompressor.DecompressAllTags, SnappyDecompressor.cs:184-347, is a single serial tag walk; a compressor that
// follows SnappyCompressor.cs:34-80 restarts its table every 65 536 input bytes, so no copy of fragment f reads output
// of fragment f-1 -- the fragments are independent once their starting tags are known).
//
// A Snappy stream carries no index: the start of tag k+1 is only known after tag k is decoded.  But "the tag that would
// start at byte j" can be decoded for EVERY byte j at once, giving next[j] (start of the following tag) and len[j]
// (output bytes the tag produces).  Walking a chain of next-pointers is pointer jumping:
//   1. one workgroup per 16 KiB chunk of the stream builds (len, next) for its 16 384 positions in LDS and runs 12
//      rounds of in-place pointer doubling, restricted to jumps that stay inside a 4 KiB sub-chunk -- afterwards
//      entry j holds (output bytes, first tag start at or after the end of j's sub-chunk) for a walk that enters at j;
//   2. the only serial step is a decoupled look-back: workgroup k waits for the true entry point of its chunk from
//      workgroup k-1 (one 64-bit word: position | output offset), follows it through its four sub-chunks (four LDS
//      reads), records the four entry points, and publishes the entry of chunk k+1.  Workgroups take their chunk
//      number from a ticket counter, so a workgroup only ever waits for one that started earlier.
// Round 5: step 2 as written above is a chain of ~0.84 us hand-offs, one per 16 KiB of stream -- 15.6 ms per GiB of output, twelve times the
// fragment decode itself.  It is now the FALLBACK.  The default takes the chain off the workgroups:
//   2a. k_tag_cand: workgroup k, with the same table in LDS, follows the walks that enter its chunk at its first 128 bytes: after 16 KiB they
//       have merged, and their (usually one) landing point in chunk k + 1 is a CANDIDATE entry of that chunk, handed to the neighbour only (no
//       chain: every workgroup publishes before it waits).  For each of its own <= 8 candidates it records what step 2 would have recorded:
//       the sub-chunk entry points and the exit, output bytes counted from the entry.
//   2b. k_tag_scan: ONE workgroup.  A chunk is a function  row -> (row of the next chunk | a position further on | end, output bytes); functions
//       compose: every thread evaluates its run of chunks for each row, thread 0 chains the runs, every thread replays its run and writes the entries.
//   2c. k_tag_fix: a landing that is no candidate (a literal longer than a chunk -- incompressible fragments -- lands in the middle of a chunk whose
//       own walks started in its body) stops the scan; one workgroup follows the true chain from there, giving each landing its row (from the tag's
//       own bytes when it leaves its chunk by itself, from the chunk's table otherwise) until the chain is on a candidate again; the scan runs
//       again (its run functions are cached: only runs that stopped at the landing are evaluated anew).  Same kernel, same workgroup, one pass per
//       incompressible region; on anything irregular, or when the passes would cost more than it (one per 417 chunks), the look-back kernel runs.
// The entry table (one entry per 4 KiB of compressed data) is searched per fragment by k_fragment_starts; the
// fragment decoder (k_decompress<.., FRAG = true>) then parses at most 4 KiB of tags before its fragment begins.
// Anything that is not a well-formed stream ending exactly at (n, declared length) marks the table irregular and the
// caller falls back to the single-wavefront decoder, which owns the error semantics.
#include "tag_index_device.h"                  // every step's body (shared with buffers_decode.hip): the kernels below are their single-block drivers

namespace {

__global__ __launch_bounds__(kThreads) void k_tag_index(const u8* __restrict__ src, u32 n, u32 hb, u32 nchunks,
                                                  u64* __restrict__ entries, u32* __restrict__ ticket, const u32* __restrict__ wanted)
{
    __shared__ u64 T[kChunk];
    __shared__ __attribute__((aligned(16))) u8 s_raw[kChunk + 16];
    __shared__ u32 s_chunk;
    if (__hip_atomic_load(wanted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;   // (the fallback: k_tag_scan found every entry among the candidates)
    if (threadIdx.x == 0) s_chunk = atomicAdd(ticket, 1u);
    __syncthreads();
    const u32 k = s_chunk;
    if (k >= nchunks) return;
    look_back_chunk(T, s_raw, src, n, hb, k, entries);
}

__global__ __launch_bounds__(kThreads) void k_tag_cand(const u8* __restrict__ src, u32 n, u32 hb, u32 nchunks, CandTable* __restrict__ tables,
                                                 CandHandoff* __restrict__ hand, u32* __restrict__ ticket)
{
    __shared__ u64 T[kChunk];
    __shared__ __attribute__((aligned(16))) u8 s_raw[kChunk + 16];
    __shared__ u32 s_chunk;
    __shared__ u32 s_land[kProbe];
    __shared__ u32 s_ncand;
    __shared__ u32 s_key[kMaxCand];
    __shared__ u32 s_next_ncand;
    __shared__ u32 s_next_key[kMaxCand];
    if (threadIdx.x == 0) s_chunk = atomicAdd(ticket, 1u);
    __syncthreads();
    const u32 k = s_chunk;
    if (k >= nchunks) return;
    cand_chunk(T, s_raw, s_land, s_ncand, s_key, s_next_ncand, s_next_key, src, n, hb, k, tables, hand);
}

// One workgroup: scan; while a landing is pending: give it (and what follows it, up to the rejoin) rows, scan again.
__global__ __launch_bounds__(kThreads) void k_tag_scan(const u8* __restrict__ src, CandTable* __restrict__ tables, u32 n, u32 hb, u32 nchunks,
                                                      u64* __restrict__ entries, ScanCtl* __restrict__ ctl, RunCache* __restrict__ cache)
{
    __shared__ __attribute__((aligned(16))) u8 pool[sizeof(FixLds) > sizeof(ScanLds) ? sizeof(FixLds) : sizeof(ScanLds)];
    __shared__ FixVars vars;
    __shared__ u32 s_final, s_more;
    if (__hip_atomic_load(&ctl->fallback, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;   // (the caller asked for the look-back pass)
    for (u32 pass = 0;; ++pass) {
        scan_pass(tables, n, hb, nchunks, entries, ctl, cache, pass >= min(kFixPasses, max(1u, nchunks / kChunksPerPass)), *reinterpret_cast<ScanLds*>(pool), s_final);
        if (threadIdx.x == 0) s_more = ctl->complete == 0 && ctl->fallback == 0 && ctl->pending != 0;
        __syncthreads();
        if (!s_more) break;
        fix_pass(src, n, hb, tables, ctl, *reinterpret_cast<FixLds*>(pool), vars);
    }
}

// One thread per output fragment: the last table entry at or before the fragment's first output byte.
__global__ __launch_bounds__(256) void k_fragment_starts(const u64* __restrict__ scanned, const u64* __restrict__ looked_back,
                                                        const u32* __restrict__ fallback, u32 nent, u32 n, u32 expected,
                                                        u32 nfrag, u64* __restrict__ in_off, u32* __restrict__ in_len,
                                                        u64* __restrict__ out_off, u32* __restrict__ out_cap,
                                                        u32* __restrict__ skip)
{
    const u32 f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nfrag) return;
    const u64* const entries = *fallback ? looked_back : scanned;
    const u32 target = f * SNP_BLOCK_SIZE;
    const FragStart fs = fragment_start(entries, nent, n, expected, target);
    out_off[f] = target;
    out_cap[f] = expected - target < SNP_BLOCK_SIZE ? expected - target : SNP_BLOCK_SIZE;
    in_off[f] = fs.ip;
    in_len[f] = fs.good ? n - fs.ip : 0u;
    skip[f] = fs.skip;
}

}  // namespace

extern "C" u32 snp_tag_index_entries(u32 n, u32 hb) { return snp_tag_chunks(n, hb) * kSubs + 1; }

// Workspace layout (all zeroed by the launch): scanned entries | look-back entries | tickets and flag | hand-offs | candidate tables.
static size_t ws_entries(u32 nent) { return (static_cast<size_t>(nent) * 8 + 63) / 64 * 64; }
extern "C" size_t snp_tag_index_workspace_bytes(u32 n, u32 hb)
{
    const u32 nent = snp_tag_index_entries(n, hb);
    const u32 nchunks = (nent - 1) / kSubs;
    return 2 * ws_entries(nent) + 64 + (static_cast<size_t>(nchunks) + 2) * sizeof(CandHandoff) + static_cast<size_t>(nchunks) * sizeof(CandTable) + 128 + sizeof(RunCache);
}

extern "C" size_t snp_tag_index_fallback_offset(u32 n, u32 hb) { return 2 * ws_entries(snp_tag_index_entries(n, hb)) + 8; }   // (ctl[2])

// The workspace holds snp_tag_index_workspace_bytes(n, hb) bytes; its first snp_tag_index_entries words are the entry table when the fallback flag is 0
// (the debug dump in capi_host.hip reads those).  Three steps, so that a caller who uploads the stream in slices can index what has arrived:
//   snp_launch_tag_index_begin   zeroes the control words;
//   snp_launch_tag_index_chunks  k_tag_cand for chunks [first, first + count), IN ORDER (the tickets number the chunks across launches); chunk k
//                                needs stream bytes [hb + k * 16 KiB, hb + (k + 1) * 16 KiB + 8) on the device (snp_tag_index_chunks_ready);
//   snp_launch_tag_index_finish  the scan, the look-back fallback, the fragment table.
namespace {
struct TagIndexLayout {
    u32 nent, nchunks;
    u64 *scanned, *looked_back;
    u32* ctl;                                                            // [0] k_tag_cand's ticket, [1] k_tag_index's, [2] the fallback flag
    CandHandoff* hand;
    CandTable* tables;
    RunCache* cache;
};
TagIndexLayout tag_index_layout(u64* work, u32 n, u32 hb)
{
    TagIndexLayout L;
    L.nent = snp_tag_index_entries(n, hb);
    L.nchunks = (L.nent - 1) / kSubs;
    u8* const w = reinterpret_cast<u8*>(work);
    L.scanned = work;
    L.looked_back = reinterpret_cast<u64*>(w + ws_entries(L.nent));
    L.ctl = reinterpret_cast<u32*>(w + 2 * ws_entries(L.nent));
    L.hand = reinterpret_cast<CandHandoff*>(L.ctl + 16);
    L.tables = reinterpret_cast<CandTable*>(reinterpret_cast<u8*>(L.hand) + (static_cast<size_t>(L.nchunks) + 2) * sizeof(CandHandoff));
    L.cache = reinterpret_cast<RunCache*>((reinterpret_cast<uintptr_t>(L.tables + L.nchunks) + 63) / 64 * 64);
    return L;
}
}  // namespace

// How many chunks of the stream are complete on the device once its first `uploaded` bytes are (of n).
extern "C" u32 snp_tag_index_chunks_ready(u32 n, u32 hb, u64 uploaded)
{
    const u32 nchunks = (snp_tag_index_entries(n, hb) - 1) / kSubs;
    if (uploaded >= n) return nchunks;
    if (uploaded < static_cast<u64>(hb) + 8) return 0;
    const u64 k = (uploaded - hb - 8) / kChunk;
    return k < nchunks ? static_cast<u32>(k) : nchunks;
}

// look_back_only: skip the candidate pass (snp_launch_tag_index_chunks / the scan do nothing) -- for streams that are mostly literals longer than a
// chunk (hardly compressed data), where the candidate pass would fail anyway and only add its 4.7 ms per GiB.
extern "C" hipError_t snp_launch_tag_index_begin(u64* work, u32 n, u32 hb, int look_back_only, hipStream_t stream)
{
    const TagIndexLayout L = tag_index_layout(work, n, hb);
    // (the candidate tables are written before they are read: only what precedes them needs zeroing)
    hipError_t e = hipMemsetAsync(work, 0, reinterpret_cast<u8*>(L.tables) - reinterpret_cast<u8*>(work), stream);
    if (e == hipSuccess && look_back_only) e = hipMemsetAsync(L.ctl + 2, 1, 4, stream);   // (any non-zero value is "wanted")
    return e;
}

extern "C" hipError_t snp_launch_tag_index_chunks(const u8* src, u32 n, u32 hb, u64* work, u32 first, u32 count, hipStream_t stream)
{
    (void)first;                                                         // (in order: the ticket counter IS the chunk number)
    if (count == 0) return hipSuccess;
    const TagIndexLayout L = tag_index_layout(work, n, hb);
    hipLaunchKernelGGL(k_tag_cand, dim3(count), dim3(kThreads), 0, stream, src, n, hb, L.nchunks, L.tables, L.hand, L.ctl);
    return hipGetLastError();
}

extern "C" hipError_t snp_launch_tag_index_finish(const u8* src, u32 n, u32 hb, u32 expected, u64* work, u64* in_off, u32* in_len,
                                                  u64* out_off, u32* out_cap, u32* skip, hipStream_t stream)
{
    const TagIndexLayout L = tag_index_layout(work, n, hb);
    const u32 nfrag = (expected + SNP_BLOCK_SIZE - 1) / SNP_BLOCK_SIZE;
    hipLaunchKernelGGL(k_tag_scan, dim3(1), dim3(kThreads), 0, stream, src, L.tables, n, hb, L.nchunks, L.scanned, reinterpret_cast<ScanCtl*>(L.ctl), L.cache);
    hipLaunchKernelGGL(k_tag_index, dim3(L.nchunks), dim3(kThreads), 0, stream, src, n, hb, L.nchunks, L.looked_back, L.ctl + 1, L.ctl + 2);
    hipLaunchKernelGGL(k_fragment_starts, dim3((nfrag + 255) / 256), dim3(256), 0, stream, L.scanned, L.looked_back, L.ctl + 2, L.nent, n, expected,
                       nfrag, in_off, in_len, out_off, out_cap, skip);
    return hipGetLastError();
}

extern "C" int snp_tag_index_look_back_only(u32 n, u32 expected) { return snp_look_back_only(n, expected); }

extern "C" hipError_t snp_launch_tag_index(const u8* src, u32 n, u32 hb, u32 expected, u64* work, u64* in_off, u32* in_len,
                                           u64* out_off, u32* out_cap, u32* skip, hipStream_t stream)
{
    const int lbo = snp_tag_index_look_back_only(n, expected);
    hipError_t e = snp_launch_tag_index_begin(work, n, hb, lbo, stream);
    if (e != hipSuccess) return e;
    if (!lbo) e = snp_launch_tag_index_chunks(src, n, hb, work, 0, (snp_tag_index_entries(n, hb) - 1) / kSubs, stream);
    if (e != hipSuccess) return e;
    return snp_launch_tag_index_finish(src, n, hb, expected, work, in_off, in_len, out_off, out_cap, skip, stream);
}
