// frame_cuts_rule_check.hip -- the rules of libsnappier_hip_frame_cuts.so (snappier_amd/csrc/frame_cuts_device.h) run on the CPU, meant to be built
// with -fsanitize=address,undefined on the host side: a stand-alone program that reads cases from a file (tests/frame_cuts_model.py,
// write_cases) and prints what the header's functions make of them, for the model to compare.  The cuts of a buffer are found the slow way, by
// the rule's own words: g of every position by cc_step (and again by cc_hash_at, which must agree), every eligible position against every
// position of its window by cc_beats_before / cc_beats_behind, the forced cuts of every gap by cc_forced_in.  Cut lists go through the encoder's
// verdict (ec_range_ok, ec_cut_ok, ec_tail_ok) and its piece arithmetic (ec_piece, ec_first_piece_from); lengths only, no data, so a buffer
// past 4 GiB costs its cut list alone.  The tables are heap blocks of exactly their sizes.  No GPU is touched.
//
//   frame_cuts_rule_check cases.bin > lines.txt
// first line: GEAR[0] GEAR[1] GEAR[2] GEAR[97] GEAR[255] g(32) of the bytes 0 .. 31
// R params-ok cuts forced bound cut...        V good pieces staging      P start:len ...      A pieces-before-offset ...      F count k0      J joined
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_cuts_device.h"

namespace {

typedef unsigned long long ull;

bool read_words(FILE* f, u64* dst, u64 n) { return n == 0 || fread(dst, sizeof(u64), n, f) == n; }

template <class T>
std::unique_ptr<T[]> exact(u64 n) { return std::unique_ptr<T[]>(new T[n]); }

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    u64 counts[4];
    if (!read_words(f, counts, 4)) return 3;
    {
        u8 ramp[32];
        for (u32 i = 0; i < 32; ++i) ramp[i] = static_cast<u8>(i);
        printf("%08x %08x %08x %08x %08x %08x\n", cc_gear(0), cc_gear(1), cc_gear(2), cc_gear(97), cc_gear(255), cc_hash_at(ramp, 32));
    }
    for (u64 i = 0; i < counts[0]; ++i) {
        u64 head[3];
        if (!read_words(f, head, 3)) return 3;
        const u32 w = static_cast<u32>(head[0]), mx = static_cast<u32>(head[1]);
        const u64 n = head[2];
        auto x = exact<u8>(n);
        if (n && fread(x.get(), 1, n, f) != n) return 3;
        auto g = exact<u32>(n + 1);
        g[0] = 0;
        for (u64 c = 0; c < n; ++c) g[c + 1] = cc_step(g[c], cc_gear(x[c]));
        for (u64 c = 0; c <= n; ++c)
            if (cc_hash_at(x.get(), c) != g[c]) { fprintf(stderr, "cc_hash_at disagrees at %llu\n", static_cast<ull>(c)); return 4; }
        std::vector<u64> marks{0}, cuts;
        for (u64 c = 0; c <= n; ++c) {
            if (!cc_eligible(c, n, w)) continue;
            bool cut = true;
            for (u64 q = c - w; q < c && cut; ++q) cut = cc_beats_before(g[c], g[q]);
            for (u64 q = c + 1; q <= c + w && cut; ++q) cut = cc_beats_behind(g[c], g[q]);
            if (cut) marks.push_back(c);
        }
        marks.push_back(n);
        u64 forced = 0;
        for (size_t k = 0; k + 1 < marks.size() && n; ++k) {
            u64 k0;
            const u64 cnt = cc_forced_in(marks[k], marks[k], marks[k + 1], mx, &k0);
            for (u64 j = 0; j < cnt; ++j) cuts.push_back(marks[k] + (k0 + j) * mx);
            forced += cnt;
            if (marks[k + 1] < n) cuts.push_back(marks[k + 1]);
        }
        printf("R %d %llu %llu %llu", cc_params_ok(w, mx) ? 1 : 0, static_cast<ull>(cuts.size()), static_cast<ull>(forced),
               static_cast<ull>(cc_cut_bound(n, w, mx)));
        for (u64 c : cuts) printf(" %llu", static_cast<ull>(c));
        printf("\n");
    }
    for (u64 i = 0; i < counts[1]; ++i) {
        u64 head[7];
        if (!read_words(f, head, 7)) return 3;
        const u64 n = head[0], lo = head[1], hi = head[2], ncuts = head[3], have = head[4], nk = head[5], na = head[6];
        auto cuts = exact<u64>(have), ks = exact<u64>(nk), ats = exact<u64>(na);
        if (!read_words(f, cuts.get(), have) || !read_words(f, ks.get(), nk) || !read_words(f, ats.get(), na) || ncuts > have) return 3;
        bool good = ec_range_ok(lo, hi, ncuts);
        u64 stage = 0;
        for (u64 k = lo; good && k < hi; ++k) {
            const u64 prev = k > lo ? cuts[k - 1] : 0;
            good = ec_cut_ok(prev, cuts[k], n);
            if (good) stage += ec_stride(cuts[k] - prev);
        }
        if (good) {
            const u64 last = hi > lo ? cuts[hi - 1] : 0;
            good = ec_tail_ok(last, n);
            if (good && n) stage += ec_stride(n - last);
        }
        printf("V %d %llu %llu\n", good ? 1 : 0, static_cast<ull>(good ? ec_pieces(lo, hi, n) : 0), static_cast<ull>(good ? stage : 0));
        if (!good) continue;
        printf("P");
        for (u64 q = 0; q < nk; ++q) {
            u64 start;
            const u32 len = ec_piece(cuts.get(), lo, hi, n, ks[q], &start);
            printf(" %llu:%u", static_cast<ull>(start), len);
        }
        printf("\nA");
        for (u64 q = 0; q < na; ++q) printf(" %llu", static_cast<ull>(ec_first_piece_from(cuts.get(), lo, hi, ats[q])));
        printf("\n");
    }
    for (u64 i = 0; i < counts[2]; ++i) {
        u64 q[4], k0;
        if (!read_words(f, q, 4)) return 3;
        const u64 cnt = cc_forced_in(q[0], q[1], q[2], static_cast<u32>(q[3]), &k0);
        printf("F %llu %llu\n", static_cast<ull>(cnt), static_cast<ull>(k0));
    }
    for (u64 i = 0; i < counts[3]; ++i) {
        u64 q[2];
        if (!read_words(f, q, 2)) return 3;
        printf("J %llu\n", static_cast<ull>(cc_sat_join(q[0], q[1])));
    }
    fclose(f);
    return 0;
}
