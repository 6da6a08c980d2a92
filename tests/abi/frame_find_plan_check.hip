// frame_find_plan_check.hip -- the planning header of the batch find (snappier_amd/csrc/frame_find_device.h) run on the CPU, meant to be built
// with -fsanitize=address,undefined on the host side: a stand-alone program that reads cases -- a batch of streams, then per case an index and
// requests with a needle length each (tests/frame_find_model.py, write_cases) -- and prints, per request, what fd_plan, fd_starts, fd_tiles,
// fd_tile and fd_row make of it.  Streams and index arrays are heap blocks of exactly their sizes, so a read past the index (beyond nentries)
// or past a stream's bytes is reported by the sanitizer.  The index is untrusted input: the cases include indexes filled with anything at all
// and windows beyond 2^32 bytes.  No GPU is touched.
//
//   frame_find_plan_check cases.bin > plans.txt
// per request: status rows bytes, and when the plan is OK: start-positions tiles first-tile-first first-tile-end last-tile-first last-tile-end
// rows-that-fail-their-check (tests/frame_find_model.py, plan_line)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_find_device.h"

namespace {

using ull = unsigned long long;

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
    u64 ns = 0, ncases = 0;
    if (!read_words(f, &ns, 1)) return 3;
    std::vector<std::unique_ptr<u8[]>> streams;
    auto lens = exact<u64>(ns);
    for (u64 b = 0; b < ns; ++b) {
        u64 n = 0;
        if (!read_words(f, &n, 1)) return 3;
        streams.push_back(exact<u8>(n));
        if (n && fread(streams.back().get(), 1, n, f) != n) return 3;
        lens[b] = n;
    }
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
            const u32 b = static_cast<u32>(q[0]), m = static_cast<u32>(q[3]);
            const FdPlan p = fd_plan(x, static_cast<u32>(ns), b, q[1], q[2], m);
            printf("%d %llu %llu", p.k.status, static_cast<ull>(p.rows), static_cast<ull>(p.bytes));
            if (p.k.status == SNP_OK) {
                const u64 starts = fd_starts(p.k.hi - p.k.lo, m), nt = fd_tiles(starts);
                u64 e[4] = {0, 0, 0, 0};
                if (nt) {
                    fd_tile(p.k.lo, starts, 0, e, e + 1);
                    fd_tile(p.k.lo, starts, nt - 1, e + 2, e + 3);
                }
                u64 bad = 0;
                for (u64 i = p.k.r0; i < p.k.r1; ++i) {
                    Hop h{};
                    bool good = false;
                    u64 at = 0;
                    const bool inside = fd_row(x, streams[b].get(), lens[b], p, i, &h, &good, &at);
                    bad += !good;
                    if (inside && (at > p.bytes || h.dec > p.bytes - at)) return 4;   // a row that may be decoded lies inside the run
                }
                printf(" %llu %llu %llu %llu %llu %llu %llu", static_cast<ull>(starts), static_cast<ull>(nt), static_cast<ull>(e[0]), static_cast<ull>(e[1]),
                       static_cast<ull>(e[2]), static_cast<ull>(e[3]), static_cast<ull>(bad));
            }
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}
