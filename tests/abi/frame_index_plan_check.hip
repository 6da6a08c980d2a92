// frame_index_plan_check.hip -- the planning header of the indexed read (snappier_amd/csrc/frame_index_device.h) run on the CPU, meant to be built
// with -fsanitize=address,undefined on the host side: a stand-alone program that reads streams, indexes and requests from a file
// (tests/frame_index_model.py, write_cases) and prints, per request, what ix_plan and ix_row_check make of it.  Streams and index arrays are heap
// blocks of exactly their sizes, so a read past the index (beyond nentries) or past a stream's bytes is reported by the sanitizer.  The index
// is untrusted input: the cases include indexes filled with anything at all.  No GPU is touched.
//
//   frame_index_plan_check cases.bin > plans.txt
// per request: status lo hi r0 r1 head last interior-rows edge-bytes interior-rows-that-fail-their-check
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_index_device.h"

namespace {

bool read_words(FILE* f, u64* dst, u64 n) { return n == 0 || fread(dst, sizeof(u64), n, f) == n; }

// a heap block of exactly n elements (n == 0: one the sanitizer lets nobody read)
template <class T>
std::unique_ptr<T[]> exact(u64 n) { return std::unique_ptr<T[]>(new T[n]); }

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    u64 ns = 0;
    if (!read_words(f, &ns, 1)) return 3;
    std::vector<std::unique_ptr<u8[]>> streams;
    std::vector<u64> lens;
    for (u64 b = 0; b < ns; ++b) {
        u64 n = 0;
        if (!read_words(f, &n, 1)) return 3;
        streams.push_back(exact<u8>(n));
        if (n && fread(streams.back().get(), 1, n, f) != n) return 3;
        lens.push_back(n);
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
            u64 q[4];
            if (!read_words(f, q, 4)) return 3;
            const u32 b = static_cast<u32>(q[0]);
            IxPlan k = ix_plan(x, static_cast<u32>(ns), b, q[1], q[2], q[3]);
            u64 cnt = 0, edge_bytes = 0, bad = 0;
            if (k.status == SNP_OK && k.r0 < k.r1) {
                const u8* const p = streams[b].get();
                Hop hh{}, ht{};
                const bool good = (!k.head || ix_row_check(x, p, lens[b], k, k.r0, false, &hh)) &&
                                  (!k.last || ix_row_check(x, p, lens[b], k, k.r1 - 1, false, &ht));
                if (good) {
                    cnt = k.interior();
                    edge_bytes = (k.head ? hh.dec : 0) + static_cast<u64>(k.last ? ht.dec : 0);
                    const u64 i0 = k.r0 + (k.head ? 1 : 0);
                    for (u64 i = i0; i < i0 + cnt; ++i) {
                        Hop h{};
                        if (i >= k.f1 || !ix_row_check(x, p, lens[b], k, i, true, &h)) ++bad;
                    }
                } else {
                    k.status = SNP_ERR_BAD_ARG;
                }
            }
            const bool ok = k.status == SNP_OK;
            printf("%d %llu %llu %llu %llu %d %d %llu %llu %llu\n", k.status, static_cast<unsigned long long>(ok ? k.lo : 0),
                   static_cast<unsigned long long>(ok ? k.hi : 0), static_cast<unsigned long long>(ok ? k.r0 : 0),
                   static_cast<unsigned long long>(ok ? k.r1 : 0), ok && k.head, ok && k.last, static_cast<unsigned long long>(cnt),
                   static_cast<unsigned long long>(edge_bytes), static_cast<unsigned long long>(bad));
        }
    }
    fclose(f);
    return 0;
}
