// frame_splice_plan_check.hip -- the planning header of the indexed splice (snappier_amd/csrc/frame_splice_device.h) run on the CPU, meant to be built
// with -fsanitize=address,undefined on the host side: a stand-alone program that reads streams, indexes and splices from a file
// (tests/frame_splice_model.py, write_cases) and prints, per stream, what fs_plan, fs_piece and fs_row_start make of it.  Streams and index
// arrays are heap blocks of exactly their sizes, so a read past the index (beyond nentries) or past a stream's bytes is reported by the
// sanitizer.  The index is untrusted input: the cases include indexes filled with anything at all.  A second kind of case gives a stream as
// NUMBERS -- its length, up to two index rows and the headers those rows point at -- so that positions, holes and inserted lengths past 4 GiB are
// planned without holding such a stream.  No GPU is touched.
//
//   frame_splice_plan_check cases.bin > plans.txt
// per stream: status splice ident head tail hl tl e0 e1 f0 rows r0 r1 p0 p1 tpos region pieces stage bound
//             | first piece: len off row-start, last piece: len off row-start
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_splice_device.h"

namespace {

bool read_words(FILE* f, u64* dst, u64 n) { return n == 0 || fread(dst, sizeof(u64), n, f) == n; }

// a heap block of exactly n elements (n == 0: one the sanitizer lets nobody read)
template <class T>
std::unique_ptr<T[]> exact(u64 n) { return std::unique_ptr<T[]>(new T[n]); }

void print_plan(const FsPlan& k, u32 cb, u64 off)
{
    FsPiece p0{0, 0}, p1{0, 0};
    u64 r0 = 0, r1 = 0;
    if (k.pieces) {
        p0 = fs_piece(k.region, cb, 0);
        p1 = fs_piece(k.region, cb, k.pieces - 1);
        r0 = fs_row_start(off, k.hl, cb, 0);
        r1 = fs_row_start(off, k.hl, cb, k.pieces - 1);
    }
    using ull = unsigned long long;
    printf("%d %d %d %d %d %u %u %u %u %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu | %u %llu %llu %u %llu %llu\n", k.status, k.splice,
           k.ident, k.head, k.tail, k.hl, k.tl, k.e0, k.e1, static_cast<ull>(k.f0), static_cast<ull>(k.rows), static_cast<ull>(k.r0),
           static_cast<ull>(k.r1), static_cast<ull>(k.p0), static_cast<ull>(k.p1), static_cast<ull>(k.tpos), static_cast<ull>(k.region),
           static_cast<ull>(k.pieces), static_cast<ull>(k.stage), static_cast<ull>(k.bound), p0.len, static_cast<ull>(p0.off), static_cast<ull>(r0),
           p1.len, static_cast<ull>(p1.off), static_cast<ull>(r1));
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
        auto first = exact<u64>(ns + 1), total = exact<u64>(ns), tail64 = exact<u64>(ns), start = exact<u64>(ne), pos = exact<u64>(ne);
        auto off = exact<u64>(ns), del = exact<u64>(ns), ins = exact<u64>(ns);
        auto tail = exact<i32>(ns);
        if (!read_words(f, first.get(), ns + 1) || !read_words(f, total.get(), ns) || !read_words(f, tail64.get(), ns) ||
            !read_words(f, start.get(), ne) || !read_words(f, pos.get(), ne) || !read_words(f, off.get(), ns) || !read_words(f, del.get(), ns) ||
            !read_words(f, ins.get(), ns))
            return 3;
        for (u64 b = 0; b < ns; ++b) tail[b] = static_cast<i32>(static_cast<u32>(tail64[b]));
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), ne};
        for (u32 b = 0; b < ns; ++b) {
            const u8* const s = streams[b].get();
            const u64 n = lens[b];
            print_plan(fs_plan(x, b, n, off[b], del[b], ins[b], cb, [&](u64 p) { return frame_hop(s, n, p); }), cb, off[b]);
        }
    }
    // a stream as numbers: n, off, del, ins, cb, total, tail, rows (0 .. 2), and per row: start, pos and the header at pos: kind (0 data, 1
    // skippable), size, dec
    u64 nnum = 0;
    if (!read_words(f, &nnum, 1)) return 3;
    for (u64 c = 0; c < nnum; ++c) {
        u64 q[18];
        if (!read_words(f, q, 18)) return 3;
        const u64 rows = q[7] < 2 ? q[7] : 2;
        auto first = exact<u64>(2), total = exact<u64>(1), start = exact<u64>(rows), pos = exact<u64>(rows);
        auto tail = exact<i32>(1);
        first[0] = 0;
        first[1] = rows;
        total[0] = q[5];
        tail[0] = static_cast<i32>(static_cast<u32>(q[6]));
        for (u64 j = 0; j < rows; ++j) { start[j] = q[8 + 5 * j]; pos[j] = q[9 + 5 * j]; }
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), rows};
        const auto hop_at = [&](u64 p) {
            const u64* const r = p == q[9] ? q + 8 : q + 13;
            Hop h{};
            h.kind = r[2] == 0 ? HOP_DATA : HOP_SKIP;
            h.type = 1;
            h.body_len = static_cast<u32>(r[3] - 4);
            h.dec = static_cast<u32>(r[4]);
            h.next = p + 4 + r[3];
            return h;
        };
        print_plan(fs_plan(x, 0, q[0], q[1], q[2], q[3], static_cast<u32>(q[4]), hop_at), static_cast<u32>(q[4]), q[1]);
    }
    fclose(f);
    return 0;
}
