// frame_update_plan_check.hip -- the planning header of the indexed write (snappier_amd/csrc/frame_update_device.h) run on the CPU, meant to be built
// with -fsanitize=address,undefined on the host side: a stand-alone program that reads streams, indexes and request lists from a file
// (tests/frame_update_model.py, write_cases) and prints, per request, what fu_plan, fu_own and fu_row_check make of it -- the requests of a list
// in order, as the plan, own and check kernels of frame_update.hip see them.  Streams, index arrays and request arrays are heap blocks of
// exactly their sizes, so a read past the index (beyond nentries), past a stream's bytes or past the request list is reported by the
// sanitizer.  The index and the list are untrusted input: the cases include both filled with anything at all.  No GPU is touched.
//
//   frame_update_plan_check cases.bin > plans.txt
// per request: status r0 r1 head last own0 owned-rows owned-bytes owned-rows-that-fail-their-check
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_update_device.h"

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
        auto rs = exact<u32>(nreq);
        auto ro = exact<u64>(nreq), rl = exact<u64>(nreq), r1s = exact<u64>(nreq);
        for (u64 r = 0; r < nreq; ++r) {
            u64 q[3];
            if (!read_words(f, q, 3)) return 3;
            rs[r] = static_cast<u32>(q[0]);
            ro[r] = q[1];
            rl[r] = q[2];
        }
        const FuRequests q{rs.get(), ro.get(), rl.get(), static_cast<u32>(nreq)};
        bool have_live = false;
        u64 last_live = 0;
        for (u32 r = 0; r < nreq; ++r) {
            FuPlan k = fu_plan(x, static_cast<u32>(ns), q, r, [&](u32 b) { return static_cast<const u8*>(streams[b].get()); }, [&](u32 b) { return lens[b]; });
            r1s[r] = k.r1;
            u64 own0 = k.r0, cnt = 0, bytes = 0, bad = 0;
            if (k.status == SNP_OK && k.r0 < k.r1) {
                const u32 b = rs[r];
                const bool has = have_live && rs[last_live] == b;
                const u64 pr1 = has ? r1s[last_live] : 0;
                const FuOwn o = fu_own(k.r0, k.r1, has, pr1);
                if (o.status != SNP_OK) k.status = o.status;
                own0 = o.own0;
                cnt = o.cnt;
                const IxPlan w = fu_window(x, b, ro[r], rl[r]);
                if (cnt) bytes = ix_row_end(x, w.f1, w.total, k.r1 - 1) - x.start[own0];
                bool has_prev = has;
                u64 prev = pr1 - 1;
                for (u64 i = own0; i < own0 + cnt; ++i) {
                    Hop h{};
                    if (!fu_row_check(x, streams[b].get(), lens[b], w, k, i, has_prev, prev, &h)) ++bad;
                    has_prev = true;
                    prev = i;
                }
                have_live = true;
                last_live = r;
            }
            printf("%d %llu %llu %d %d %llu %llu %llu %llu\n", k.status, static_cast<unsigned long long>(k.r0), static_cast<unsigned long long>(k.r1),
                   k.head, k.last, static_cast<unsigned long long>(own0), static_cast<unsigned long long>(cnt), static_cast<unsigned long long>(bytes),
                   static_cast<unsigned long long>(bad));
        }
    }
    fclose(f);
    return 0;
}
