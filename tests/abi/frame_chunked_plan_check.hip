// frame_chunked_plan_check.hip -- the slot arithmetic of snp_frame_encode_chunked_batch (snappier_amd/csrc/frame_chunked_device.h) run on the CPU,
// meant to be built with -fsanitize=address,undefined on the host side: a stand-alone program that reads cases from a file
// (tests/frame_chunked_model.py, write_cases) -- a chunk size, max_chunks, the staging stride, buffer lengths and their verdicts, and slots to
// ask about -- and prints what fc_chunks, fc_slot, fc_stage_off, fc_row, fc_group and fc_team make of them.  Lengths only, no data: a buffer of
// 2^32 + 5 bytes costs nothing here, and an overflowing 32-bit product is what UBSan and the expected lines are for.  The scans are plain
// loops (the device's are scan_tiles.h); the tables are heap blocks of exactly their sizes.  No GPU is touched.
//
//   frame_chunked_plan_check cases.bin > plans.txt
// per case: slots-needed rows-of-the-OK-buffers group team; per slot: owner(-1: none) len k off stage-offset row start
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../../snappier_amd/csrc/frame_chunked_device.h"

namespace {

bool read_words(FILE* f, u64* dst, u64 n) { return n == 0 || fread(dst, sizeof(u64), n, f) == n; }

template <class T>
std::unique_ptr<T[]> exact(u64 n) { return std::unique_ptr<T[]>(new T[n]); }

typedef unsigned long long ull;

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    u64 ncases = 0;
    if (!read_words(f, &ncases, 1)) return 3;
    for (u64 i = 0; i < ncases; ++i) {
        u64 head[4], nslots = 0;
        if (!read_words(f, head, 4)) return 3;
        const u32 cb = static_cast<u32>(head[0]), max_chunks = static_cast<u32>(head[1]), nb = static_cast<u32>(head[3]);
        const u64 stride = head[2];
        auto in_len = exact<u64>(nb), status = exact<u64>(nb), first = exact<u64>(nb + 1), ok_first = exact<u64>(nb + 1);
        if (!read_words(f, in_len.get(), nb) || !read_words(f, status.get(), nb) || !read_words(f, &nslots, 1)) return 3;
        first[0] = ok_first[0] = 0;
        for (u32 b = 0; b < nb; ++b) {
            const u64 n = fc_chunks(in_len[b], cb);
            first[b + 1] = first[b] + n;
            ok_first[b + 1] = ok_first[b] + (status[b] == SNP_OK ? n : 0);
        }
        const u32 group = fc_group(cb);
        printf("%llu %llu %u %u\n", static_cast<ull>(first[nb]), static_cast<ull>(ok_first[nb]), group, fc_team(group));
        auto slots = exact<u64>(nslots);
        if (!read_words(f, slots.get(), nslots)) return 3;
        for (u64 q = 0; q < nslots; ++q) {
            const u32 c = static_cast<u32>(slots[q]);
            const FcSlot s = fc_slot(first.get(), in_len.get(), nb, max_chunks, cb, c);
            FcRow r{0, 0};
            if (s.owner != kFcNone && status[s.owner] == SNP_OK) r = fc_row(ok_first[s.owner], s.k, cb);
            printf("%d %u %llu %llu %llu %llu %llu\n", s.owner == kFcNone ? -1 : static_cast<int>(s.owner), s.len, static_cast<ull>(s.k),
                   static_cast<ull>(s.off), static_cast<ull>(fc_stage_off(c, stride)), static_cast<ull>(r.row), static_cast<ull>(r.start));
        }
    }
    fclose(f);
    return 0;
}
