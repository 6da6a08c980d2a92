// frame_digest_plan_check.hip -- the arithmetic and the planning header of the batch digest (snappier_amd/csrc/frame_digest_device.h) run on the
// CPU, meant to be built with -fsanitize=address,undefined on the host side: a stand-alone program that reads (crc, byte count) pairs from one
// file and streams, indexes and requests from another (tests/frame_digest_model.py, write_shifts; tests/frame_index_model.py, write_cases) and
// prints what crc_shift makes of every pair -- counts of 2^32 bytes and more included -- and, per request, what dg_plan and dg_row_term make of
// it.  Streams and index arrays are heap blocks of exactly their sizes, so a read past the index (beyond nentries) or past a stream's bytes is
// reported by the sanitizer.  The index is untrusted input: the cases include indexes filled with anything at all.  No GPU is touched.
//
//   frame_digest_plan_check shifts.bin cases.bin > plans.txt
// per pair:    crc_shift(c, n)
// per request: status lo hi interior-rows edge-bytes interior-rows-that-fail-their-check XOR-of-the-interior-terms (0 if a row fails)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_digest_device.h"

namespace {

using ull = unsigned long long;

bool read_words(FILE* f, u64* dst, u64 n) { return n == 0 || fread(dst, sizeof(u64), n, f) == n; }

// a heap block of exactly n elements (n == 0: one the sanitizer lets nobody read)
template <class T>
std::unique_ptr<T[]> exact(u64 n) { return std::unique_ptr<T[]>(new T[n]); }

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s shifts.bin cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    u64 nshift = 0;
    if (!read_words(f, &nshift, 1)) return 3;
    for (u64 i = 0; i < nshift; ++i) {
        u64 q[2];
        if (!read_words(f, q, 2)) return 3;
        printf("%u\n", crc_shift(static_cast<u32>(q[0]), q[1]));
    }
    fclose(f);
    f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    u64 ns = 0;
    if (!read_words(f, &ns, 1)) return 3;
    std::vector<std::unique_ptr<u8[]>> streams;
    auto lens = exact<u64>(ns), offs = exact<u64>(ns);
    for (u64 b = 0; b < ns; ++b) {
        u64 n = 0;
        if (!read_words(f, &n, 1)) return 3;
        streams.push_back(exact<u8>(n));
        if (n && fread(streams.back().get(), 1, n, f) != n) return 3;
        lens[b] = n;
        offs[b] = 0;
    }
    u64 ncases = 0;
    if (!read_words(f, &ncases, 1)) return 3;
    for (u64 c = 0; c < ncases; ++c) {
        u64 ne = 0, nreq = 0;
        if (!read_words(f, &ne, 1)) return 3;
        auto first = exact<u64>(ns + 1), total = exact<u64>(ns), tail64 = exact<u64>(ns), start = exact<u64>(ne), pos = exact<u64>(ne);
        auto tail = exact<i32>(ns);
        if (!read_words(f, first.get(), ns + 1) || !read_words(f, total.get(), ns) || !read_words(f, tail64.get(), ns) ||
            !read_words(f, start.get(), ne) || !read_words(f, pos.get(), ne) || !read_words(f, &nreq, 1))
            return 3;
        for (u64 b = 0; b < ns; ++b) tail[b] = static_cast<i32>(static_cast<u32>(tail64[b]));
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), ne};
        for (u64 r = 0; r < nreq; ++r) {
            u64 q[4];                                                   // stream, off, len, (a capacity: the digest has none)
            if (!read_words(f, q, 4)) return 3;
            const u32 b = static_cast<u32>(q[0]);
            // (every stream is its own heap block: the plan gets the block of stream b as `in` and offsets of 0)
            const DgPlan d = dg_plan(x, b < ns ? streams[b].get() : nullptr, offs.get(), lens.get(), static_cast<u32>(ns), b, q[1], q[2]);
            u64 edge_bytes = 0, bad = 0;
            u32 sum = 0;
            const bool ok = d.k.status == SNP_OK;
            if (ok) {
                edge_bytes = (d.k.head ? d.hh.dec : 0) + static_cast<u64>(d.k.last ? d.ht.dec : 0);
                const u64 i0 = d.k.r0 + (d.k.head ? 1 : 0);
                for (u64 i = i0; i < i0 + d.interior; ++i) {
                    u32 term = 0;
                    if (dg_row_term(x, streams[b].get(), lens[b], d.k, i, &term)) sum ^= term;
                    else ++bad;
                }
            }
            printf("%d %llu %llu %llu %llu %llu %u\n", d.k.status, static_cast<ull>(ok ? d.k.lo : 0), static_cast<ull>(ok ? d.k.hi : 0),
                   static_cast<ull>(d.interior), static_cast<ull>(edge_bytes), static_cast<ull>(bad), bad ? 0u : sum);
        }
    }
    fclose(f);
    return 0;
}
