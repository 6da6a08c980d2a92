// frame_append_plan_check.hip -- the planning header of the indexed append (snappier_amd/csrc/frame_append_device.h) run on the CPU, meant to be built
// with -fsanitize=address,undefined on the host side: a stand-alone program that reads streams, indexes and appended lengths from a file
// (tests/frame_append_model.py, write_cases) and prints, per stream, what fa_plan, fa_piece and fa_row_start make of it.  Streams and index
// arrays are heap blocks of exactly their sizes, so a read past the index (beyond nentries) or past a stream's bytes is reported by the
// sanitizer.  The index is untrusted input: the cases include indexes filled with anything at all.  A second kind of case gives a stream as
// NUMBERS -- its length, one index row and the header that row points at -- so that positions and appended lengths past 4 GiB are planned without
// holding such a stream.  No GPU is touched.
//
//   frame_append_plan_check cases.bin > plans.txt
// per stream: status append reopen ident d fill f0 rows cut rest fresh bound | first piece: len off row-start, last piece: len off row-start
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_append_device.h"

namespace {

bool read_words(FILE* f, u64* dst, u64 n) { return n == 0 || fread(dst, sizeof(u64), n, f) == n; }

// a heap block of exactly n elements (n == 0: one the sanitizer lets nobody read)
template <class T>
std::unique_ptr<T[]> exact(u64 n) { return std::unique_ptr<T[]>(new T[n]); }

void print_plan(const FaPlan& k, u32 cb, u64 total)
{
    FaPiece p0{0, 0}, p1{0, 0};
    u64 r0 = 0, r1 = 0;
    if (k.fresh) {
        p0 = fa_piece(k.rest, k.fill, cb, 0);
        p1 = fa_piece(k.rest, k.fill, cb, k.fresh - 1);
        r0 = fa_row_start(total, k.fill, cb, 0);
        r1 = fa_row_start(total, k.fill, cb, k.fresh - 1);
    }
    using ull = unsigned long long;
    printf("%d %d %d %d %u %u %llu %llu %llu %llu %llu %llu | %u %llu %llu %u %llu %llu\n", k.status, k.append, k.reopen, k.ident, k.d, k.fill,
           static_cast<ull>(k.f0), static_cast<ull>(k.rows), static_cast<ull>(k.cut), static_cast<ull>(k.rest), static_cast<ull>(k.fresh),
           static_cast<ull>(k.bound), p0.len, static_cast<ull>(p0.off), static_cast<ull>(r0), p1.len, static_cast<ull>(p1.off), static_cast<ull>(r1));
}

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
        u64 head[2] = {0, 0};
        if (!read_words(f, head, 2)) return 3;
        const u64 ne = head[0];
        const u32 cb = static_cast<u32>(head[1]);
        auto first = exact<u64>(ns + 1), total = exact<u64>(ns), tail64 = exact<u64>(ns), start = exact<u64>(ne), pos = exact<u64>(ne), src_len = exact<u64>(ns);
        auto tail = exact<i32>(ns);
        if (!read_words(f, first.get(), ns + 1) || !read_words(f, total.get(), ns) || !read_words(f, tail64.get(), ns) ||
            !read_words(f, start.get(), ne) || !read_words(f, pos.get(), ne) || !read_words(f, src_len.get(), ns))
            return 3;
        for (u64 b = 0; b < ns; ++b) tail[b] = static_cast<i32>(static_cast<u32>(tail64[b]));
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), ne};
        for (u32 b = 0; b < ns; ++b) {
            const u8* const s = streams[b].get();
            const u64 n = lens[b];
            print_plan(fa_plan(x, b, n, src_len[b], cb, [&](u64 p) { return frame_hop(s, n, p); }), cb, total[b]);
        }
    }
    // a stream as numbers: n, src_len, cb, total, start, pos, tail, rows (0 | 1), and the header at pos: kind (0 data, 1 skippable), size, dec
    u64 nnum = 0;
    if (!read_words(f, &nnum, 1)) return 3;
    for (u64 c = 0; c < nnum; ++c) {
        u64 q[11];
        if (!read_words(f, q, 11)) return 3;
        const u64 rows = q[7] ? 1 : 0;
        auto first = exact<u64>(2), total = exact<u64>(1), start = exact<u64>(rows), pos = exact<u64>(rows);
        auto tail = exact<i32>(1);
        first[0] = 0;
        first[1] = rows;
        total[0] = q[3];
        tail[0] = static_cast<i32>(static_cast<u32>(q[6]));
        if (rows) { start[0] = q[4]; pos[0] = q[5]; }
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), rows};
        const auto hop_at = [&](u64 p) {
            Hop h{};
            h.kind = q[8] == 0 ? HOP_DATA : HOP_SKIP;
            h.type = 1;
            h.body_len = static_cast<u32>(q[9] - 4);
            h.dec = static_cast<u32>(q[10]);
            h.next = p + 4 + q[9];
            return h;
        };
        print_plan(fa_plan(x, 0, q[0], q[1], static_cast<u32>(q[2]), hop_at), static_cast<u32>(q[2]), q[3]);
    }
    fclose(f);
    return 0;
}
