// frame_verify_plan_check.hip -- the rules of libsnappier_hip_frame_verify.so (snappier_amd/csrc/frame_verify_device.h) run on the CPU, meant to be
// built with -fsanitize=address,undefined on the host side: a stand-alone program that reads cases from a file (tests/frame_verify_model.py,
// write_cases) and prints what the header's functions make of them, for the model to compare.  One part needs no model and is checked here
// against brute force: the rounds (every row has one round and one slot, a slot ends inside rows_per_round * stride <= scratch_cap, the rows
// of a round have slots of their own).  The verdict of a stream walks its rows with vf_row over dd_stream, as the kernel does, over indexes
// filled with anything at all; what its rows add up to is joined in row order and again from four interleaved parts, as a workgroup's
// wavefronts would hold them, and both must agree.  The program knows no decoder: a row whose round would tell counts as SNP_OK.  The planner
// (rp_begin, rp_plan) reads no stream: its cases are numbers alone, past 4 GiB too.  No GPU is touched.
//
//   frame_verify_plan_check cases.bin > lines.txt
// G ok cases      R stride per_round rounds off off off      V row_status ...      S status:nbad:first_bad:bad_bytes:flags ... | d_result
// P plan_status src:off:len ... ; ... | d_result
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../snappier_amd/csrc/frame_verify_device.h"

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

bool rounds_all(u64* cases)
{
    for (u32 n = 0; n < 4000; ++n) {
        const u32 slot = n < 64 ? n + 1 : n < 128 ? 65536 - (n - 64) : static_cast<u32>(next_rand() % 65536) + 1;
        const u64 ne = next_rand() % 700;
        const u64 stride = (static_cast<u64>(slot) + 15) / 16 * 16;
        const u64 cap = n % 5 == 0 ? next_rand() : n % 5 == 1 ? stride * (next_rand() % 9) + next_rand() % stride : n % 5 == 2 ? stride - 1 : next_rand() % (stride * 800);
        const VfRounds r = vf_rounds(slot, cap, ne);
        if (r.stride != stride || r.stride < slot || r.stride % 16 || r.per_round > ne || r.per_round * r.stride > cap) return false;
        if ((cap >= stride && ne) != (r.per_round > 0) || (r.per_round == 0) != (r.rounds == 0)) return false;
        if (r.per_round && (r.per_round < ne && (r.per_round + 1) * r.stride <= cap)) return false;     // the most rows that fit
        std::vector<u64> seen(r.rounds * r.per_round, 0);
        for (u64 i = 0; r.per_round && i < ne; ++i) {
            const u64 q = i / r.per_round, off = vf_slot_off(r, i);
            if (q >= r.rounds || off % r.stride || off + r.stride > r.per_round * r.stride) return false;
            if (seen[q * r.per_round + off / r.stride]++) return false;
        }
        if (r.rounds && (r.rounds - 1) * r.per_round >= ne) return false;                                // no empty round
        ++*cases;
    }
    const VfRounds big = vf_rounds(65536, ~0ull, kVfMaxRows);
    return big.per_round == kVfMaxRows && big.rounds == 1 && vf_rounds(1, 15, 9).rounds == 0 && vf_rounds(1, 16, 9).rounds == 9;
}

bool same(const VfAcc& a, const VfAcc& b)
{
    return a.looked == b.looked && a.bad == b.bad && a.first == b.first && a.bad_bytes == b.bad_bytes && a.ok_bytes == b.ok_bytes &&
           a.longest == b.longest && a.unverified == b.unverified;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    u64 cases = 0;
    if (!rounds_all(&cases)) { fprintf(stderr, "the rounds disagree with brute force after %llu cases\n", static_cast<ull>(cases)); return 4; }
    printf("G ok %llu\n", static_cast<ull>(cases));
    u64 counts[4];
    if (!read_words(f, counts, 4)) return 3;
    for (u64 i = 0; i < counts[0]; ++i) {
        u64 q[3];
        if (!read_words(f, q, 3)) return 3;
        const VfRounds r = vf_rounds(static_cast<u32>(q[0]), q[1], q[2]);
        const bool any = r.per_round && q[2];
        printf("R %llu %llu %llu %llu %llu %llu\n", static_cast<ull>(r.stride), static_cast<ull>(r.per_round), static_cast<ull>(r.rounds),
               static_cast<ull>(any ? vf_slot_off(r, 0) : 0), static_cast<ull>(any ? vf_slot_off(r, q[2] / 2) : 0),
               static_cast<ull>(any ? vf_slot_off(r, q[2] - 1) : 0));
    }
    const u64 ns = counts[1];
    std::vector<std::unique_ptr<u8[]>> streams;
    auto in_len = exact<u64>(ns);
    for (u64 b = 0; b < ns; ++b) {
        if (!read_words(f, &in_len[b], 1)) return 3;
        streams.push_back(exact<u8>(in_len[b]));
        if (in_len[b] && fread(streams.back().get(), 1, in_len[b], f) != in_len[b]) return 3;
    }
    for (u64 c = 0; c < counts[2]; ++c) {
        u64 head[3];
        if (!read_words(f, head, 3)) return 3;
        const u64 ne = head[0];
        const u32 slot_bytes = static_cast<u32>(head[1]);
        auto first = exact<u64>(ns + 1), total = exact<u64>(ns), tail64 = exact<u64>(ns), start = exact<u64>(ne), pos = exact<u64>(ne);
        auto tail = exact<i32>(ns);
        if (!read_words(f, first.get(), ns + 1) || !read_words(f, total.get(), ns) || !read_words(f, tail64.get(), ns) ||
            !read_words(f, start.get(), ne) || !read_words(f, pos.get(), ne))
            return 3;
        for (u64 b = 0; b < ns; ++b) tail[b] = static_cast<i32>(static_cast<u32>(tail64[b]));
        const FrameIndex x{first.get(), start.get(), pos.get(), total.get(), tail.get(), ne};
        const VfRounds rounds = vf_rounds(slot_bytes, head[2], ne);
        auto row_status = exact<i32>(ne);
        auto len = exact<u64>(ne);
        auto checked = exact<u8>(ne);
        for (u64 i = 0; i < ne; ++i) row_status[i] = kVfSkipped, len[i] = 0, checked[i] = 0;
        std::vector<i32> status(ns);
        std::vector<u32> flags(ns);
        std::vector<VfAcc> per(ns, vf_none());
        VfAcc all = vf_none();
        u64 before = 0, ok = 0;
        for (u64 b = 0; b < ns; ++b) {
            const u8* const s = streams[b].get();
            const CcSeg k = dd_stream(x, in_len.get(), static_cast<u32>(b), before);
            before = dd_first(x, b) > before ? dd_first(x, b) : before;
            flags[b] = fr_ident(s, in_len[b]) ? 0u : kVfNoIdent;
            status[b] = k.status;
            if (k.status != SNP_OK) continue;
            for (u64 i = k.r0; i < k.r1; ++i) {
                const VfRow r = vf_row(x, k, i, slot_bytes, rounds, [&](u64 p) { return frame_hop(s, k.n, p); });
                if (r.checked && r.h.dec != r.len) return 4;            // a checked row decodes to what the index says
                if (r.status == SNP_OK && vf_slot_off(rounds, i) + r.h.dec > rounds.per_round * rounds.stride) return 4;   // ... inside the scratch
                row_status[i] = r.status;
                len[i] = r.len;
                checked[i] = r.checked ? 1 : 0;
            }
            // what the rows add up to: in row order, and from four interleaved parts
            u64 f0, rows;
            fr_rows(x, static_cast<u32>(b), &f0, &rows);
            if (f0 != k.r0 || f0 + rows != k.r1) return 4;
            VfAcc part[4] = {vf_none(), vf_none(), vf_none(), vf_none()}, joined = vf_none();
            for (u64 i = f0; i < f0 + rows; ++i) {
                vf_add(&per[b], i, row_status[i], checked[i] != 0, len[i]);
                vf_add(&part[(i - f0) % 4], i, row_status[i], checked[i] != 0, len[i]);
            }
            for (u32 q : {2u, 0u, 3u, 1u}) vf_join(&joined, part[q]);
            if (!same(joined, per[b])) return 4;
            if (per[b].first != kVfNone) status[b] = row_status[per[b].first];
            vf_join(&all, per[b]);
        }
        printf("V");
        for (u64 i = 0; i < ne; ++i) printf(" %d", row_status[i]);
        printf("\nS");
        for (u64 b = 0; b < ns; ++b) {
            ok += status[b] == SNP_OK ? 1 : 0;
            printf(" %d:%llu:%llu:%llu:%u", status[b], static_cast<ull>(per[b].bad), static_cast<ull>(per[b].first), static_cast<ull>(per[b].bad_bytes),
                   flags[b]);
        }
        printf(" | %llu %llu %llu %llu %llu %llu %llu %llu\n", static_cast<ull>(all.looked), static_cast<ull>(all.bad), static_cast<ull>(all.ok_bytes),
               static_cast<ull>(ok), static_cast<ull>(all.longest), static_cast<ull>(all.unverified), static_cast<ull>(rounds.rounds),
               static_cast<ull>(all.bad_bytes));
    }
    for (u64 c = 0; c < counts[3]; ++c) {
        u64 head[4];
        if (!read_words(f, head, 4)) return 3;
        const u64 pns = head[0], ne = head[1], nrep = head[2], npairs = head[3];
        auto first = exact<u64>(pns + 1), total = exact<u64>(pns), tail64 = exact<u64>(pns), start = exact<u64>(ne), rs64 = exact<u64>(ne),
             rep_total = exact<u64>(nrep), rtail64 = exact<u64>(nrep);
        auto tail = exact<i32>(pns), rep_tail = exact<i32>(nrep), row_status = exact<i32>(ne);
        if (!read_words(f, first.get(), pns + 1) || !read_words(f, total.get(), pns) || !read_words(f, tail64.get(), pns) ||
            !read_words(f, start.get(), ne) || !read_words(f, rs64.get(), ne) || !read_words(f, rep_total.get(), nrep) ||
            !read_words(f, rtail64.get(), nrep))
            return 3;
        for (u64 b = 0; b < pns; ++b) tail[b] = static_cast<i32>(static_cast<u32>(tail64[b]));
        for (u64 b = 0; b < nrep; ++b) rep_tail[b] = static_cast<i32>(static_cast<u32>(rtail64[b]));
        for (u64 i = 0; i < ne; ++i) row_status[i] = static_cast<i32>(static_cast<u32>(rs64[i]));
        const FrameIndex x{first.get(), start.get(), nullptr, total.get(), tail.get(), ne};
        RpCount sum{};
        u64 ok = 0;
        printf("P");
        for (u64 j = 0; j < npairs; ++j) {
            u64 pair[2];
            if (!read_words(f, pair, 2)) return 3;
            const u32 s = static_cast<u32>(pair[0]), t = static_cast<u32>(pair[1]);
            const i32 st = rp_begin(x, static_cast<u32>(pns), rep_total.get(), rep_tail.get(), static_cast<u32>(nrep), s, t);
            printf(" %d", st);
            if (st == SNP_OK) {
                u64 listed = 0;
                const RpCount cnt = rp_plan(x, row_status.get(), static_cast<u32>(pns), s, t, [&](u32 src, u64 off, u64 n) {
                    printf(" %u:%llu:%llu", src, static_cast<ull>(off), static_cast<ull>(n));
                    ++listed;
                });
                if (listed != cnt.segs) return 4;
                sum.segs += cnt.segs;
                sum.taken += cnt.taken;
                sum.kept += cnt.kept;
                ++ok;
            }
            printf(" ;");
        }
        printf(" | %llu %llu %llu %llu\n", static_cast<ull>(sum.segs), static_cast<ull>(ok), static_cast<ull>(sum.taken), static_cast<ull>(sum.kept));
    }
    fclose(f);
    return 0;
}
