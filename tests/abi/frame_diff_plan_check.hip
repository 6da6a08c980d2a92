// frame_diff_plan_check.hip -- the planning header of the batch diff (snappier_amd/csrc/frame_diff_device.h) run on the CPU, meant to be built
// with -fsanitize=address,undefined on the host side: a stand-alone program that reads cases -- two sides, each a batch of streams with an
// index, and requests (tests/frame_diff_model.py, write_cases) -- and prints, per request, what df_side, df_scan_seq, df_pieces and
// df_piece_side make of it.  Streams and index arrays are heap blocks of exactly their sizes, so a read past the index (beyond nentries) or
// past a stream's bytes is reported by the sanitizer.  Both indexes are untrusted input: the cases include indexes filled with anything at all
// and windows beyond 2^32 bytes.  No GPU is touched.
//
//   frame_diff_plan_check cases.bin > plans.txt
// per request: status-a status-b, and when both are OK: n, then per direction asked for: bad-a bad-b have-cut span-differs and for each of the two
// pieces t0 len and per side row0 nrows bytes off (tests/frame_diff_model.py, plan_line)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_diff_device.h"

namespace {

using ull = unsigned long long;

bool read_words(FILE* f, u64* dst, u64 n) { return n == 0 || fread(dst, sizeof(u64), n, f) == n; }

// a heap block of exactly n elements (n == 0: one the sanitizer lets nobody read)
template <class T>
std::unique_ptr<T[]> exact(u64 n) { return std::unique_ptr<T[]>(new T[n]); }

struct SideData {
    u64 ns = 0, ne = 0;
    std::vector<std::unique_ptr<u8[]>> streams;
    std::unique_ptr<u64[]> lens, offs, first, total, start, pos;
    std::unique_ptr<i32[]> tail;
    FrameIndex x{};
    bool read(FILE* f)
    {
        if (!read_words(f, &ns, 1)) return false;
        lens = exact<u64>(ns);
        offs = exact<u64>(ns);
        for (u64 b = 0; b < ns; ++b) {
            u64 n = 0;
            if (!read_words(f, &n, 1)) return false;
            streams.push_back(exact<u8>(n));
            if (n && fread(streams.back().get(), 1, n, f) != n) return false;
            lens[b] = n;
            offs[b] = 0;
        }
        if (!read_words(f, &ne, 1)) return false;
        first = exact<u64>(ns + 1);
        total = exact<u64>(ns);
        start = exact<u64>(ne);
        pos = exact<u64>(ne);
        tail = exact<i32>(ns);
        auto tail64 = exact<u64>(ns);
        if (!read_words(f, first.get(), ns + 1) || !read_words(f, total.get(), ns) || !read_words(f, tail64.get(), ns) ||
            !read_words(f, start.get(), ne) || !read_words(f, pos.get(), ne))
            return false;
        for (u64 b = 0; b < ns; ++b) tail[b] = static_cast<i32>(static_cast<u32>(tail64[b]));
        x = FrameIndex{first.get(), start.get(), pos.get(), total.get(), tail.get(), ne};
        return true;
    }
    // (every stream is its own heap block: the plan gets the block of stream b as `in` and offsets of 0)
    DfSide side(u32 b, u64 off, u64 len) const { return df_side(x, b < ns ? streams[b].get() : nullptr, offs.get(), lens.get(), static_cast<u32>(ns), b, off, len); }
};

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    u64 ncases = 0;
    if (!read_words(f, &ncases, 1)) return 3;
    for (u64 c = 0; c < ncases; ++c) {
        SideData sa, sb;
        u64 head[2];
        if (!sa.read(f) || !sb.read(f) || !read_words(f, head, 2)) return 3;
        const u32 flags = static_cast<u32>(head[0]);
        for (u64 r = 0; r < head[1]; ++r) {
            u64 q[6];
            if (!read_words(f, q, 6)) return 3;
            const DfSide A = sa.side(static_cast<u32>(q[0]), q[1], q[2]), B = sb.side(static_cast<u32>(q[3]), q[4], q[5]);
            printf("%d %d", A.k.status, B.k.status);
            if (A.k.status != SNP_OK || B.k.status != SNP_OK) { printf("\n"); continue; }
            const u64 n = A.len() < B.len() ? A.len() : B.len();
            printf(" %llu", static_cast<ull>(n));
            const bool ex = flags & kDiffExact;
            auto gb = exact<u32>(B.rows() + 1);
            for (u32 dir = 0; dir < 2; ++dir) {
                if (!(flags & (dir ? kDiffSuffix : kDiffPrefix))) continue;
                const DfScan s = df_scan_seq(sa.x, A, sb.x, B, dir, n, !ex && n > 0, gb.get());
                const bool bad = s.bad_a || s.bad_b;
                printf(" %d %d %d %d", s.bad_a, s.bad_b, s.have0 && !bad, s.diff && !bad);
                DfPiece pc[2] = {};
                if (!bad) df_pieces(s, df_need_rows(sa.x, A, dir, n), df_need_rows(sb.x, B, dir, n), n, ex, pc);
                for (u32 k = 0; k < 2; ++k) {
                    u64 v[8];
                    df_piece_side(sa.x, A, dir, pc[k].a0, pc[k].a1, pc[k].t0, pc[k].len, v, v + 1, v + 2, v + 3);
                    df_piece_side(sb.x, B, dir, pc[k].b0, pc[k].b1, pc[k].t0, pc[k].len, v + 4, v + 5, v + 6, v + 7);
                    printf(" %llu %llu", static_cast<ull>(pc[k].t0), static_cast<ull>(pc[k].len));
                    for (u64 w : v) printf(" %llu", static_cast<ull>(w));
                }
            }
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}
