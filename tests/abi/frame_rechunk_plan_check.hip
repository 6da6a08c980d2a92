// frame_rechunk_plan_check.hip -- the planning header of the indexed rechunk (snappier_amd/csrc/frame_rechunk_device.h) run on the CPU, meant to be
// built with -fsanitize=address,undefined on the host side: a stand-alone program that reads streams and indexes from a file
// (tests/frame_rechunk_model.py, write_cases) and prints, per stream, what fr_plan, the fr_count_* functions, fr_piece and fr_slot_len make of it.
// Streams and index arrays are heap blocks of exactly their sizes, so a read past the index (beyond nentries) or past a stream's bytes is
// reported by the sanitizer.  The index is untrusted input: the cases include indexes filled with anything at all.  A second kind of case gives a
// stream as NUMBERS -- its length, up to two index rows and the headers those rows point at -- so that positions and totals past 4 GiB are planned
// without holding such a stream.  No GPU is touched.
//
//   frame_rechunk_plan_check cases.bin > plans.txt
// per stream: status work last f0 rows dirty dbytes pieces rebuilt kept bound | what it asks of the four bounds
//             | first piece: kept row at len, last piece: kept row at len, the last rebuilt slot's length
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_rechunk_device.h"

namespace {

bool read_words(FILE* f, u64* dst, u64 n) { return n == 0 || fread(dst, sizeof(u64), n, f) == n; }

// a heap block of exactly n elements (n == 0: one the sanitizer lets nobody read)
template <class T>
std::unique_ptr<T[]> exact(u64 n) { return std::unique_ptr<T[]>(new T[n]); }

void print_plan(const FrPlan& k, const FrameIndex& x, u64 total, u32 cb, bool all)
{
    FrPiece p0{}, p1{};
    u32 last = 0;
    if (k.work && k.pieces) {
        p0 = fr_piece(x, k.f0, k.f0 + k.rows, total, cb, all, 0);
        p1 = fr_piece(x, k.f0, k.f0 + k.rows, total, cb, all, k.pieces - 1);
        last = k.rebuilt ? fr_slot_len(k.last, k.rebuilt, k.pieces, total, cb, k.rebuilt - 1) : 0;
    }
    using ull = unsigned long long;
    printf("%d %d %d %llu %llu %llu %llu %llu %llu %llu %llu | %llu %llu %llu %llu | %d %llu %llu %u %d %llu %llu %u %u\n", k.status, k.work, k.last,
           static_cast<ull>(k.f0), static_cast<ull>(k.rows), static_cast<ull>(k.dirty), static_cast<ull>(k.dbytes), static_cast<ull>(k.pieces),
           static_cast<ull>(k.rebuilt), static_cast<ull>(k.kept), static_cast<ull>(k.bound), static_cast<ull>(fr_count_dirty(k)),
           static_cast<ull>(fr_count_slots(k)), static_cast<ull>(fr_count_stage(k)), static_cast<ull>(fr_count_rows(k)), p0.kept,
           static_cast<ull>(p0.row), static_cast<ull>(p0.at), p0.len, p1.kept, static_cast<ull>(p1.row), static_cast<ull>(p1.at), p1.len, last);
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
        u64 head[3] = {0, 0, 0};
        if (!read_words(f, head, 3)) return 3;
        const u64 ne = head[0];
        const u32 cb = static_cast<u32>(head[1]);
        const bool all = (head[2] & kFrRewriteAll) != 0;
        auto first = exact<u64>(ns + 1), total = exact<u64>(ns), tail64 = exact<u64>(ns), start = exact<u64>(ne), pos = exact<u64>(ne);
        auto tail = exact<i32>(ns);
        if (!read_words(f, first.get(), ns + 1) || !read_words(f, total.get(), ns) || !read_words(f, tail64.get(), ns) ||
            !read_words(f, start.get(), ne) || !read_words(f, pos.get(), ne))
            return 3;
        for (u64 b = 0; b < ns; ++b) tail[b] = static_cast<i32>(static_cast<u32>(tail64[b]));
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), ne};
        for (u32 b = 0; b < ns; ++b) {
            const u8* const s = streams[b].get();
            const u64 n = lens[b];
            print_plan(fr_plan(x, b, n, cb, all, fr_ident(s, n), [&](u64 p) { return frame_hop(s, n, p); }), x, total[b], cb, all);
        }
    }
    // a stream as numbers: n, cb, flags, total, tail, rows (0 .. 2), ident, and per row: start, pos and the header at pos: kind (0 data, 1
    // skippable), size, dec
    u64 nnum = 0;
    if (!read_words(f, &nnum, 1)) return 3;
    for (u64 c = 0; c < nnum; ++c) {
        u64 q[17];
        if (!read_words(f, q, 17)) return 3;
        const u64 rows = q[5] < 2 ? q[5] : 2;
        auto first = exact<u64>(2), total = exact<u64>(1), start = exact<u64>(rows), pos = exact<u64>(rows);
        auto tail = exact<i32>(1);
        first[0] = 0;
        first[1] = rows;
        total[0] = q[3];
        tail[0] = static_cast<i32>(static_cast<u32>(q[4]));
        for (u64 j = 0; j < rows; ++j) { start[j] = q[7 + 5 * j]; pos[j] = q[8 + 5 * j]; }
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), rows};
        const auto hop_at = [&](u64 p) {
            const u64* const r = p == q[8] ? q + 7 : q + 12;
            Hop h{};
            h.kind = r[2] == 0 ? HOP_DATA : HOP_SKIP;
            h.type = 1;
            h.body_len = static_cast<u32>(r[3] - 4);
            h.dec = static_cast<u32>(r[4]);
            h.next = p + 4 + r[3];
            return h;
        };
        const bool all = (q[2] & kFrRewriteAll) != 0;
        print_plan(fr_plan(x, 0, q[0], static_cast<u32>(q[1]), all, q[6] != 0, hop_at), x, q[3], static_cast<u32>(q[1]), all);
    }
    fclose(f);
    return 0;
}
