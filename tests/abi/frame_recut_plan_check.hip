// frame_recut_plan_check.hip -- the planning header of the indexed recut (snappier_amd/csrc/frame_recut_device.h) run on the CPU, meant to be built
// with -fsanitize=address,undefined on the host side: a stand-alone program that reads streams, indexes and cut lists from a file
// (tests/frame_recut_model.py, write_cases) and prints, per stream, what rx_plan, the rx_count_* functions, rx_piece and the maps between the
// rebuilt pieces and the dirty rows make of it.  Streams, index arrays and cut lists are heap blocks of exactly their sizes, so a read past the
// index (beyond nentries), past the list (beyond ncuts) or past a stream's bytes is reported by the sanitizer.  Both the index and the list are
// untrusted input: the cases include arrays filled with anything at all.  A second kind of case gives a stream as NUMBERS -- its length, up to two
// index rows, the headers those rows point at and up to three cuts -- so that positions, totals and cuts past 4 GiB are planned without holding
// such a stream.  No GPU is touched.
//
//   frame_recut_plan_check cases.bin > plans.txt
// per stream: status work f0 rows dirty dbytes pieces rebuilt copied kept cbytes bound | what it asks of the bounds (and the decoded part)
//             | first piece: kept row at len, last piece: kept row at len | first and last rebuilt piece: piece, place among the decoded rows, len
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_recut_device.h"

namespace {

bool read_words(FILE* f, u64* dst, u64 n) { return n == 0 || fread(dst, sizeof(u64), n, f) == n; }

// a heap block of exactly n elements (n == 0: one the sanitizer lets nobody read)
template <class T>
std::unique_ptr<T[]> exact(u64 n) { return std::unique_ptr<T[]>(new T[n]); }

struct Slot { u64 piece, place; u32 len; };

// the m-th rebuilt piece through the dirty rows, as the kernels find it: the table of the stream's dirty rows (where each starts, where it is
// decoded to, the rebuilt pieces that start in the rows before it), the last row with no more than m before it, and back again
template <class HopAt>
Slot slot_of(const RxPlan& k, const FrameIndex& x, u64 n, u64 total, const u64* cuts, u64 lo, u64 hi, bool all, u64 m, HopAt hop_at)
{
    std::vector<u64> dstart, place, pfirst;
    u64 bytes = 0, pcs = 0;
    for (u64 i = k.f0; i < k.f0 + k.rows; ++i) {
        const FrRow r = rx_row(x, k.f0, k.f0 + k.rows, total, n, cuts, lo, hi, all, i, hop_at);
        if (!r.ok || r.clean) continue;
        dstart.push_back(r.start);
        place.push_back(bytes);
        pfirst.push_back(pcs);
        bytes += r.len;
        pcs += rx_row_pieces(cuts, lo, hi, r.start, r.len);
    }
    if (pcs != k.rebuilt || bytes != k.dbytes) { fprintf(stderr, "the dirty rows do not hold the rebuilt pieces\n"); exit(4); }
    const u64 t = ix_first_where(0, pfirst.size(), [&](u64 q) { return pfirst[q] > m; });
    if (t == 0) { fprintf(stderr, "no dirty row for a rebuilt piece\n"); exit(4); }
    Slot s{};
    s.piece = rx_piece_of_slot(cuts, lo, hi, dstart[t - 1], pfirst[t - 1], m);
    u64 at;
    s.len = ec_piece(cuts, lo, hi, total, s.piece, &at);
    s.place = rx_place(place[t - 1], dstart[t - 1], at);
    // ... and the way back, as the row kernel goes it: the last dirty row that starts at or below the piece
    const u64 t2 = ix_first_where(0, dstart.size(), [&](u64 q) { return dstart[q] > at; });
    if (t2 == 0 || rx_slot_of_piece(cuts, lo, hi, dstart[t2 - 1], pfirst[t2 - 1], s.piece) != m || rx_piece(x, k.f0, k.f0 + k.rows, total, cuts, lo, hi, all, s.piece).kept ||
        s.place + s.len > bytes) {
        fprintf(stderr, "slot %llu and piece %llu do not map onto each other\n", static_cast<unsigned long long>(m), static_cast<unsigned long long>(s.piece));
        exit(4);
    }
    return s;
}

template <class HopAt>
void print_plan(const RxPlan& k, const FrameIndex& x, u64 n, u64 total, const u64* cuts, u64 lo, u64 hi, bool all, HopAt hop_at)
{
    RxPiece p0{}, p1{};
    Slot s0{}, s1{};
    if (k.work && k.pieces) {
        p0 = rx_piece(x, k.f0, k.f0 + k.rows, total, cuts, lo, hi, all, 0);
        p1 = rx_piece(x, k.f0, k.f0 + k.rows, total, cuts, lo, hi, all, k.pieces - 1);
        if (k.rebuilt) {
            s0 = slot_of(k, x, n, total, cuts, lo, hi, all, 0, hop_at);
            s1 = slot_of(k, x, n, total, cuts, lo, hi, all, k.rebuilt - 1, hop_at);
        }
    }
    using ull = unsigned long long;
    printf("%d %d %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu | %llu %llu %llu %llu %llu | %d %llu %llu %u %d %llu %llu %u | %llu %llu %u %llu %llu %u\n",
           k.status, k.work, static_cast<ull>(k.f0), static_cast<ull>(k.rows), static_cast<ull>(k.dirty), static_cast<ull>(k.dbytes),
           static_cast<ull>(k.pieces), static_cast<ull>(k.rebuilt), static_cast<ull>(k.copied), static_cast<ull>(k.kept), static_cast<ull>(k.cbytes),
           static_cast<ull>(k.bound), static_cast<ull>(rx_count_dirty(k)), static_cast<ull>(rx_count_slots(k)), static_cast<ull>(rx_count_stage(k)),
           static_cast<ull>(rx_count_dec(k)), static_cast<ull>(rx_count_rows(k)), p0.kept, static_cast<ull>(p0.row), static_cast<ull>(p0.at), p0.len,
           p1.kept, static_cast<ull>(p1.row), static_cast<ull>(p1.at), p1.len, static_cast<ull>(s0.piece), static_cast<ull>(s0.place), s0.len,
           static_cast<ull>(s1.piece), static_cast<ull>(s1.place), s1.len);
    if (k.work && rx_count_stage(k) > rx_stage_bound(k.dbytes, k.rebuilt)) { fprintf(stderr, "the documented staging bound does not hold\n"); exit(4); }
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
        const u64 ne = head[0], ncuts = head[1];
        const bool all = (head[2] & kRxRewriteAll) != 0;
        auto first = exact<u64>(ns + 1), total = exact<u64>(ns), tail64 = exact<u64>(ns), start = exact<u64>(ne), pos = exact<u64>(ne);
        auto cut_first = exact<u64>(ns + 1), cuts = exact<u64>(ncuts);
        auto tail = exact<i32>(ns);
        if (!read_words(f, first.get(), ns + 1) || !read_words(f, total.get(), ns) || !read_words(f, tail64.get(), ns) ||
            !read_words(f, start.get(), ne) || !read_words(f, pos.get(), ne) || !read_words(f, cut_first.get(), ns + 1) ||
            !read_words(f, cuts.get(), ncuts))
            return 3;
        for (u64 b = 0; b < ns; ++b) tail[b] = static_cast<i32>(static_cast<u32>(tail64[b]));
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), ne};
        for (u32 b = 0; b < ns; ++b) {
            const u8* const s = streams[b].get();
            const u64 n = lens[b];
            const auto hop_at = [&](u64 p) { return frame_hop(s, n, p); };
            print_plan(rx_plan(x, b, n, cut_first.get(), cuts.get(), ncuts, all, fr_ident(s, n), hop_at), x, n, total[b], cuts.get(), cut_first[b],
                       cut_first[b + 1], all, hop_at);
        }
    }
    // a stream as numbers: n, flags, total, tail, rows (0 .. 2), ident, per row: start, pos and the header at pos: kind (0 data, 1 skippable),
    // size, dec; then the cuts: how many (0 .. 3) and the three
    u64 nnum = 0;
    if (!read_words(f, &nnum, 1)) return 3;
    for (u64 c = 0; c < nnum; ++c) {
        u64 q[20];
        if (!read_words(f, q, 20)) return 3;
        const u64 rows = q[4] < 2 ? q[4] : 2, nc = q[16] < 3 ? q[16] : 3;
        auto first = exact<u64>(2), total = exact<u64>(1), start = exact<u64>(rows), pos = exact<u64>(rows), cut_first = exact<u64>(2), cuts = exact<u64>(nc);
        auto tail = exact<i32>(1);
        first[0] = 0;
        first[1] = rows;
        cut_first[0] = 0;
        cut_first[1] = nc;
        total[0] = q[2];
        tail[0] = static_cast<i32>(static_cast<u32>(q[3]));
        for (u64 j = 0; j < rows; ++j) { start[j] = q[6 + 5 * j]; pos[j] = q[7 + 5 * j]; }
        for (u64 j = 0; j < nc; ++j) cuts[j] = q[17 + j];
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), rows};
        const auto hop_at = [&](u64 p) {
            const u64* const r = p == q[7] ? q + 6 : q + 11;
            Hop h{};
            h.kind = r[2] == 0 ? HOP_DATA : HOP_SKIP;
            h.type = 1;
            h.body_len = static_cast<u32>(r[3] - 4);
            h.dec = static_cast<u32>(r[4]);
            h.next = p + 4 + r[3];
            return h;
        };
        const bool all = (q[1] & kRxRewriteAll) != 0;
        print_plan(rx_plan(x, 0, q[0], cut_first.get(), cuts.get(), nc, all, q[5] != 0, hop_at), x, q[0], q[2], cuts.get(), 0, nc, all, hop_at);
    }
    fclose(f);
    return 0;
}
