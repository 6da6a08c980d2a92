// frame_edit_plan_check.hip -- the planning header of the indexed edit (snappier_amd/csrc/frame_edit_device.h, on top of fs_plan of
// frame_splice_device.h) run on the CPU, meant to be built with -fsanitize=address,undefined on the host side: a stand-alone program that reads
// streams, indexes and edit lists from a file (tests/frame_edit_model.py, write_cases) and prints, per stream, what fe_csr makes of its list and,
// per named edit, what fs_plan, fe_linked and fe_verdict make of it, with the running sums kept the way the device's scans keep them (the
// inserted bytes as the sum of their low and the sum of their high halves, the deleted bytes modulo 2^64).  Streams, index arrays and edit
// arrays are heap blocks of exactly their sizes, so a read past one of them is reported by the sanitizer.  The index and ed_first are untrusted
// input: the cases include arrays filled with anything at all.  A second kind of case gives a stream as NUMBERS -- its length, up to two index
// rows and the headers those rows point at, and up to three edits -- so that positions and lengths past 4 GiB are planned without holding such a
// stream.  No GPU is touched.
//
//   frame_edit_plan_check cases.bin > plans.txt
// per stream: S b e0 e1 ok; per named edit of a stream whose list is sound: E e verdict linked |H| |T|
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_edit_device.h"

namespace {

bool read_words(FILE* f, u64* dst, u64 n) { return n == 0 || fread(dst, sizeof(u64), n, f) == n; }

// a heap block of exactly n elements (n == 0: one the sanitizer lets nobody read)
template <class T>
std::unique_ptr<T[]> exact(u64 n) { return std::unique_ptr<T[]>(new T[n]); }

// the edits [e0, e1) of stream b of n bytes
template <class HopAt>
void run_stream(const FrameIndex& x, u32 b, u64 n, u64 e0, u64 e1, const u64* off, const u64* del, const u64* ins, u32 cb, HopAt hop_at)
{
    using ull = unsigned long long;
    bool have = false;
    FeEdit prev{};
    u64 ins_hi = 0, ins_lo = 0, del_mod = 0;
    for (u64 e = e0; e < e1; ++e) {
        if (!fe_named(del[e], ins[e])) continue;
        const FsPlan k = fs_plan(x, b, n, off[e], del[e], ins[e], cb, hop_at);
        const FeEdit me = fe_edit(k, off[e], del[e]);
        ins_lo += ins[e] & 0xffffffffu;
        ins_hi += ins[e] >> 32;
        del_mod += del[e];
        const i32 v = fe_verdict(me, have ? &prev : nullptr, x.total[b], ins_hi, ins_lo, del_mod);
        const bool ln = have && fe_linked(prev, me);
        printf("E %llu %d %d %u %u\n", static_cast<ull>(e), v, ln, ln ? 0u : k.hl, k.tl);
        prev = me;
        have = true;
    }
}

}  // namespace

int main(int argc, char** argv)
{
    using ull = unsigned long long;
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
        const u64 ne = head[0], nedits = head[2];
        const u32 cb = static_cast<u32>(head[1]);
        auto first = exact<u64>(ns + 1), total = exact<u64>(ns), tail64 = exact<u64>(ns), start = exact<u64>(ne), pos = exact<u64>(ne);
        auto ed_first = exact<u64>(ns + 1), off = exact<u64>(nedits), del = exact<u64>(nedits), ins = exact<u64>(nedits);
        auto tail = exact<i32>(ns);
        if (!read_words(f, first.get(), ns + 1) || !read_words(f, total.get(), ns) || !read_words(f, tail64.get(), ns) ||
            !read_words(f, start.get(), ne) || !read_words(f, pos.get(), ne) || !read_words(f, ed_first.get(), ns + 1) ||
            !read_words(f, off.get(), nedits) || !read_words(f, del.get(), nedits) || !read_words(f, ins.get(), nedits))
            return 3;
        for (u64 b = 0; b < ns; ++b) tail[b] = static_cast<i32>(static_cast<u32>(tail64[b]));
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), ne};
        bool backwards = false;                                         // (the device: a scan over the lists that run backwards)
        for (u32 b = 0; b < ns; ++b) {
            u64 e0, e1;
            backwards = !fe_csr(ed_first.get(), nedits, b, &e0, &e1) || backwards;
            printf("S %u %llu %llu %d\n", b, static_cast<ull>(e0), static_cast<ull>(e1), !backwards);
            if (backwards) continue;
            const u8* const s = streams[b].get();
            const u64 n = lens[b];
            run_stream(x, b, n, e0, e1, off.get(), del.get(), ins.get(), cb, [&](u64 p) { return frame_hop(s, n, p); });
        }
    }
    // a stream as numbers: n, cb, total, tail, rows (0 .. 2), per row: start, pos and the header at pos: kind (0 data, 1 skippable), size, dec;
    // then the edits: how many (0 .. 3), and off, del, ins of each
    u64 nnum = 0;
    if (!read_words(f, &nnum, 1)) return 3;
    for (u64 c = 0; c < nnum; ++c) {
        u64 q[25];
        if (!read_words(f, q, 25)) return 3;
        const u64 rows = q[4] < 2 ? q[4] : 2, nedits = q[15] < 3 ? q[15] : 3;
        auto first = exact<u64>(2), total = exact<u64>(1), start = exact<u64>(rows), pos = exact<u64>(rows), ed_first = exact<u64>(2);
        auto off = exact<u64>(nedits), del = exact<u64>(nedits), ins = exact<u64>(nedits);
        auto tail = exact<i32>(1);
        first[0] = 0;
        first[1] = rows;
        ed_first[0] = 0;
        ed_first[1] = nedits;
        total[0] = q[2];
        tail[0] = static_cast<i32>(static_cast<u32>(q[3]));
        for (u64 j = 0; j < rows; ++j) { start[j] = q[5 + 5 * j]; pos[j] = q[6 + 5 * j]; }
        for (u64 j = 0; j < nedits; ++j) { off[j] = q[16 + 3 * j]; del[j] = q[17 + 3 * j]; ins[j] = q[18 + 3 * j]; }
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), rows};
        const auto hop_at = [&](u64 p) {
            const u64* const r = p == q[6] ? q + 5 : q + 10;
            Hop h{};
            h.kind = r[2] == 0 ? HOP_DATA : HOP_SKIP;
            h.type = 1;
            h.body_len = static_cast<u32>(r[3] - 4);
            h.dec = static_cast<u32>(r[4]);
            h.next = p + 4 + r[3];
            return h;
        };
        u64 e0, e1;
        const bool ok = fe_csr(ed_first.get(), nedits, 0, &e0, &e1);
        printf("S 0 %llu %llu %d\n", static_cast<ull>(e0), static_cast<ull>(e1), ok);
        run_stream(x, 0, q[0], e0, e1, off.get(), del.get(), ins.get(), static_cast<u32>(q[1]), hop_at);
    }
    fclose(f);
    return 0;
}
