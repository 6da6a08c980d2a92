// frame_compose_plan_check.hip -- the planning header of the indexed compose (snappier_amd/csrc/frame_compose_device.h) run on the CPU, meant to be
// built with -fsanitize=address,undefined on the host side: a stand-alone program that reads streams, indexes and segment lists from a file
// (tests/frame_compose_model.py, write_cases) and prints, per segment, what cc_plan, the cc_seg_* functions and cc_row make of it, and per output
// what cc_segs does.  Streams, index arrays and segment arrays are heap blocks of exactly their sizes, so a read past the index (beyond
// nentries), past the segment list or past a stream's bytes is reported by the sanitizer.  Both are untrusted input: the cases include arrays
// filled with anything at all.  A second kind of case gives a source as NUMBERS -- its length, up to two index rows and the headers those rows
// point at -- so that positions and totals past 4 GiB are planned without holding such a stream.  No GPU is touched.
//
//   frame_compose_plan_check cases.bin > plans.txt
// per segment: status head tail r0 r1 hdec tdec hlen tlen hskip hp tp kept kbytes | edges pieces stage rows bytes bound
//              | its first row: kept tail row slot from len at | its last row, the same
// per output:  ok s0 s1
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_compose_device.h"

namespace {

using ull = unsigned long long;

bool read_words(FILE* f, u64* dst, u64 n) { return n == 0 || fread(dst, sizeof(u64), n, f) == n; }

// a heap block of exactly n elements (n == 0: one the sanitizer lets nobody read)
template <class T>
std::unique_ptr<T[]> exact(u64 n) { return std::unique_ptr<T[]>(new T[n]); }

void print_row(const CcRow& r)
{
    printf(" %d %d %llu %llu %llu %u %llu", r.kept, r.tail, static_cast<ull>(r.row), static_cast<ull>(r.slot), static_cast<ull>(r.from), r.len,
           static_cast<ull>(r.at));
}

void print_seg(const CcSeg& k, const FrameIndex& x, u32 cb)
{
    printf("%d %d %d %llu %llu %u %u %u %u %llu %llu %llu %llu %llu | %llu %llu %llu %llu %llu %llu |", k.status, k.head, k.tail, static_cast<ull>(k.r0),
           static_cast<ull>(k.r1), k.hdec, k.tdec, k.hlen, k.tlen, static_cast<ull>(k.hskip), static_cast<ull>(k.hp), static_cast<ull>(k.tp),
           static_cast<ull>(k.kept), static_cast<ull>(k.kbytes), static_cast<ull>(cc_seg_edges(k)), static_cast<ull>(cc_seg_pieces(k)),
           static_cast<ull>(cc_seg_stage(k)), static_cast<ull>(cc_seg_rows(k)), static_cast<ull>(cc_seg_bytes(k)), static_cast<ull>(cc_seg_bound(k)));
    const u64 rows = k.hp + k.tp + k.kept;
    CcRow first{}, last{};
    if (rows) {
        first = cc_row(x, k.r0, k.head, k.lo, k.hp, k.kept, k.hskip, k.hlen, k.tlen, cb, 0);
        last = cc_row(x, k.r0, k.head, k.lo, k.hp, k.kept, k.hskip, k.hlen, k.tlen, cb, rows - 1);
    }
    print_row(first);
    printf(" |");
    print_row(last);
    printf("\n");
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
    auto lens = exact<u64>(ns);
    for (u64 b = 0; b < ns; ++b) {
        u64 n = 0;
        if (!read_words(f, &n, 1)) return 3;
        streams.push_back(exact<u8>(n));
        if (n && fread(streams.back().get(), 1, n, f) != n) return 3;
        lens[b] = n;
    }
    u64 ncases = 0;
    if (!read_words(f, &ncases, 1)) return 3;
    for (u64 c = 0; c < ncases; ++c) {
        u64 head[4] = {0, 0, 0, 0};
        if (!read_words(f, head, 4)) return 3;
        const u64 ne = head[0], nout = head[2], nsegs = head[3];
        const u32 cb = static_cast<u32>(head[1]);
        auto first = exact<u64>(ns + 1), total = exact<u64>(ns), tail64 = exact<u64>(ns), start = exact<u64>(ne), pos = exact<u64>(ne);
        auto seg_first = exact<u64>(nout + 1), seg_stream = exact<u64>(nsegs), seg_off = exact<u64>(nsegs), seg_len = exact<u64>(nsegs);
        auto tail = exact<i32>(ns);
        if (!read_words(f, first.get(), ns + 1) || !read_words(f, total.get(), ns) || !read_words(f, tail64.get(), ns) ||
            !read_words(f, start.get(), ne) || !read_words(f, pos.get(), ne) || !read_words(f, seg_first.get(), nout + 1) ||
            !read_words(f, seg_stream.get(), nsegs) || !read_words(f, seg_off.get(), nsegs) || !read_words(f, seg_len.get(), nsegs))
            return 3;
        for (u64 b = 0; b < ns; ++b) tail[b] = static_cast<i32>(static_cast<u32>(tail64[b]));
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), ne};
        for (u64 g = 0; g < nsegs; ++g)
            print_seg(cc_plan(x, lens.get(), static_cast<u32>(ns), static_cast<u32>(seg_stream[g]), seg_off[g], seg_len[g], cb,
                              [&](u32 b, u64 p) { return frame_hop(streams[b].get(), lens[b], p); }),
                      x, cb);
        for (u32 j = 0; j < nout; ++j) {
            u64 s0, s1;
            const bool ok = cc_segs(seg_first.get(), static_cast<u32>(nsegs), j, &s0, &s1);
            printf("%d %llu %llu\n", ok, static_cast<ull>(s0), static_cast<ull>(s1));
        }
    }
    // a source as numbers: n, cb, off, len, total, tail, rows (0 .. 2), and per row: start, pos and the header at pos: kind (0 data, 1
    // skippable), size, dec
    u64 nnum = 0;
    if (!read_words(f, &nnum, 1)) return 3;
    for (u64 c = 0; c < nnum; ++c) {
        u64 q[17];
        if (!read_words(f, q, 17)) return 3;
        const u64 rows = q[6] < 2 ? q[6] : 2;
        auto first = exact<u64>(2), total = exact<u64>(1), start = exact<u64>(rows), pos = exact<u64>(rows), n = exact<u64>(1);
        auto tail = exact<i32>(1);
        first[0] = 0;
        first[1] = rows;
        total[0] = q[4];
        n[0] = q[0];
        tail[0] = static_cast<i32>(static_cast<u32>(q[5]));
        for (u64 j = 0; j < rows; ++j) { start[j] = q[7 + 5 * j]; pos[j] = q[8 + 5 * j]; }
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), rows};
        const auto hop_at = [&](u32, u64 p) {
            const u64* const r = p == q[8] ? q + 7 : q + 12;
            Hop h{};
            h.kind = r[2] == 0 ? HOP_DATA : HOP_SKIP;
            h.type = 1;
            h.body_len = static_cast<u32>(r[3] - 4);
            h.dec = static_cast<u32>(r[4]);
            h.next = p + 4 + r[3];
            return h;
        };
        print_seg(cc_plan(x, n.get(), 1, 0, q[2], q[3], static_cast<u32>(q[1]), hop_at), x, static_cast<u32>(q[1]));
    }
    fclose(f);
    return 0;
}
