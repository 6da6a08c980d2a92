// frame_dedup_plan_check.hip -- the rules of libsnappier_hip_frame_dedup.so (snappier_amd/csrc/frame_dedup_device.h) run on the CPU, meant to be
// built with -fsanitize=address,undefined on the host side: a stand-alone program that reads cases from a file (tests/frame_dedup_model.py,
// write_cases) and prints what the header's functions make of them, for the model to compare.  Two parts need no model and are checked here
// against brute force: the compare of two chunks (dd_same against memcmp, every length up to 300 and a few long ones, at every pair of
// alignments mod 4, equal and with one byte changed at every place of short chunks and at the ends and the middle of long ones, in heap blocks
// of exactly the chunks' sizes so that a read past an end is seen), and the table (keys inserted in descending and in shuffled row order by
// dd_slot with a linear probe and a minimum per slot: every row's leader is the lowest row with its key, found by looking at every row).
// The verdict of a stream walks its rows with cc_add over dd_stream, as the kernel does, over indexes filled with anything at all.
// No GPU is touched.
//
//   frame_dedup_plan_check cases.bin > lines.txt
// C ok pairs      T ok rows      K key slots slot      B src off begins      V status:rows:chunk-bytes ...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_dedup_device.h"

namespace {

typedef unsigned long long ull;

bool read_words(FILE* f, u64* dst, u64 n) { return n == 0 || fread(dst, sizeof(u64), n, f) == n; }

template <class T>
std::unique_ptr<T[]> exact(u64 n) { return std::unique_ptr<T[]>(new T[n]); }

u64 g_rand = 0x9e3779b97f4a7c15ull;
u64 next_rand()
{
    g_rand ^= g_rand << 13;
    g_rand ^= g_rand >> 7;
    g_rand ^= g_rand << 17;
    return g_rand;
}

// one pair: chunks of n bytes at alignments sa and sb inside blocks that end with them; `at` < n: that byte differs
bool compare_case(u64 n, u32 sa, u32 sb, u64 at, u64* pairs)
{
    auto a = exact<u8>(sa + n), b = exact<u8>(sb + n);
    for (u64 i = 0; i < n; ++i) a[sa + i] = b[sb + i] = static_cast<u8>(next_rand());
    if (at < n) b[sb + at] ^= static_cast<u8>(1u << (next_rand() % 8));
    const bool want = n == 0 || memcmp(a.get() + sa, b.get() + sb, n) == 0;
    ++*pairs;
    if (dd_same(a.get() + sa, n, b.get() + sb, n) != want) return false;
    return n == 0 || !dd_same(a.get() + sa, n, b.get() + sb, n - 1);    // (chunks of different lengths are never the same)
}

bool compare_all(u64* pairs)
{
    std::vector<u64> lens;
    for (u64 n = 0; n <= 300; ++n) lens.push_back(n);
    for (u64 n : {4095ull, 4096ull, 4100ull, 65536ull + 8, 76500ull}) lens.push_back(n);
    for (u64 n : lens)
        for (u32 sa = 0; sa < 4; ++sa)
            for (u32 sb = 0; sb < 4; ++sb) {
                if (n > 300 && sa > 1 && sb > 1) continue;
                if (!compare_case(n, sa, sb, n, pairs)) return false;
                if (n <= 70) {
                    if (sa != 1 && sa != sb) continue;
                    for (u64 at = 0; at < n; ++at)
                        if (!compare_case(n, sa, sb, at, pairs)) return false;
                } else {
                    for (u64 at : {u64(0), u64(1), u64(15), u64(16), n / 2, n - 17, n - 16, n - 2, n - 1})
                        if (!compare_case(n, sa, sb, at, pairs)) return false;
                }
            }
    return true;
}

// rows with few distinct keys and with many, inserted in the order `order`: -> the leader of every row
std::vector<u32> leaders(const std::vector<u64>& keys, const std::vector<u32>& order)
{
    const u64 slots = dd_slots(keys.size()), mask = slots - 1;
    std::vector<u64> tkey(slots, kDdEmpty);
    std::vector<u32> trow(slots, kDdNoRow), slot(keys.size(), 0);
    for (u32 r : order) {
        u64 s = dd_slot(keys[r], mask);
        for (u64 n = 0; n < slots; ++n, s = (s + 1) & mask)
            if (tkey[s] == kDdEmpty || tkey[s] == keys[r]) {
                tkey[s] = keys[r];
                trow[s] = r < trow[s] ? r : trow[s];
                slot[r] = static_cast<u32>(s);
                break;
            }
    }
    std::vector<u32> out(keys.size());
    for (size_t r = 0; r < keys.size(); ++r) out[r] = trow[slot[r]];
    return out;
}

bool table_all(u64* rows)
{
    for (u32 distinct : {1u, 2u, 7u, 1000u, 0u}) {
        for (u32 n : {1u, 2u, 63u, 64u, 65u, 5000u}) {
            std::vector<u64> keys(n);
            for (u32 r = 0; r < n; ++r) {
                const u64 v = distinct ? next_rand() % distinct : next_rand();
                keys[r] = dd_key(static_cast<u32>(v % 65536) + 1, static_cast<u32>(v * 0x9e3779b1u));
            }
            std::vector<u32> brute(n);
            for (u32 r = 0; r < n; ++r) {
                brute[r] = r;
                for (u32 q = 0; q < r; ++q)
                    if (keys[q] == keys[r]) { brute[r] = q; break; }
            }
            std::vector<u32> down(n), mixed(n);
            for (u32 r = 0; r < n; ++r) down[r] = n - 1 - r, mixed[r] = r;
            for (u32 r = n; r > 1; --r) std::swap(mixed[r - 1], mixed[next_rand() % r]);
            if (leaders(keys, down) != brute || leaders(keys, mixed) != brute) return false;
            if (dd_slots(n) < 2ull * n || (dd_slots(n) & (dd_slots(n) - 1)) || dd_slots(n) < 64) return false;
            *rows += n;
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    u64 pairs = 0, rows = 0;
    if (!compare_all(&pairs)) { fprintf(stderr, "dd_same disagrees with memcmp after %llu pairs\n", static_cast<ull>(pairs)); return 4; }
    printf("C ok %llu\n", static_cast<ull>(pairs));
    if (!table_all(&rows)) { fprintf(stderr, "the table's leaders disagree with brute force\n"); return 4; }
    printf("T ok %llu\n", static_cast<ull>(rows));
    u64 counts[4];
    if (!read_words(f, counts, 4)) return 3;
    for (u64 i = 0; i < counts[0]; ++i) {
        u64 q[3];
        if (!read_words(f, q, 3)) return 3;
        const u64 key = dd_key(static_cast<u32>(q[0]), static_cast<u32>(q[1])), slots = dd_slots(q[2]);
        printf("K %llu %llu %llu\n", static_cast<ull>(key), static_cast<ull>(slots), static_cast<ull>(dd_slot(key, slots - 1)));
    }
    for (u64 i = 0; i < counts[1]; ++i) {
        u64 q[8];
        if (!read_words(f, q, 8)) return 3;
        const DdSrc cur = dd_source(static_cast<u32>(q[1]), static_cast<u32>(q[2]), q[3], q[4]);
        const bool b = dd_begins(q[0] != 0, DdSrc{static_cast<u32>(q[5]), q[6]}, q[7], cur);
        printf("B %u %llu %d\n", cur.src, static_cast<ull>(cur.off), b ? 1 : 0);
    }
    const u64 ns = counts[2];
    std::vector<std::unique_ptr<u8[]>> streams;
    auto in_len = exact<u64>(ns);
    for (u64 b = 0; b < ns; ++b) {
        if (!read_words(f, &in_len[b], 1)) return 3;
        streams.push_back(exact<u8>(in_len[b]));
        if (in_len[b] && fread(streams.back().get(), 1, in_len[b], f) != in_len[b]) return 3;
    }
    for (u64 i = 0; i < counts[3]; ++i) {
        u64 ne;
        if (!read_words(f, &ne, 1)) return 3;
        auto first = exact<u64>(ns + 1), total = exact<u64>(ns), tail64 = exact<u64>(ns), start = exact<u64>(ne), pos = exact<u64>(ne);
        auto tail = exact<i32>(ns);
        if (!read_words(f, first.get(), ns + 1) || !read_words(f, total.get(), ns) || !read_words(f, tail64.get(), ns) ||
            !read_words(f, start.get(), ne) || !read_words(f, pos.get(), ne))
            return 3;
        for (u64 b = 0; b < ns; ++b) tail[b] = static_cast<i32>(static_cast<u32>(tail64[b]));
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), ne};
        printf("V");
        u64 before = 0;
        for (u64 b = 0; b < ns; ++b) {
            const CcSeg k = dd_stream(x, in_len.get(), static_cast<u32>(b), before);
            CcAcc acc{};
            if (k.status == SNP_OK)
                for (u64 r = k.r0; r < k.r1; ++r) {
                    const u32 bad = acc.bad;
                    cc_add(&acc, x, k, r, [&](u64 p) { return frame_hop(streams[b].get(), k.n, p); });
                    // a row that passed: the CRC field read from the header's bytes is the hop's
                    if (!bad && !acc.bad && dd_crc_field(streams[b].get() + pos[r]) != frame_hop(streams[b].get(), k.n, pos[r]).crc) return 4;
                }
            const i32 verdict = k.status != SNP_OK ? k.status : acc.bad ? SNP_ERR_BAD_ARG : SNP_OK;
            printf(" %d:%llu:%llu", verdict, static_cast<ull>(verdict == SNP_OK ? acc.kept : 0), static_cast<ull>(verdict == SNP_OK ? acc.kbytes : 0));
            before = dd_first(x, b) > before ? dd_first(x, b) : before;
        }
        printf("\n");
    }
    fclose(f);
    return 0;
}
