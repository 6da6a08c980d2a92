// frame_digest_device.h -- the arithmetic and the per-request planning of the batch digest (snp_frame_digest_indexed_batch, frame_digest.hip):
// CRC-32C of a window of what a seekable framed stream decodes to, combined from the CRCs its chunk headers carry.  __host__ __device__
// throughout, so that the same code runs on the CPU under sanitizers (tests/abi/frame_digest_plan_check.hip) and behind snp_crc32c_combine.
//
// CRC-32C is GF(2)-linear: with crc(A) the plain CRC (init and final xor 0xFFFFFFFF), crc(A || B) = shift(crc(A), |B|) ^ crc(B), where
// shift(c, n) = c * x^(8n) mod P on REFLECTED 32-bit values (bit 31 is x^0), P = 0x82F63B78.  Hence for pieces that tile [lo, hi), piece i
// ending at end_i:   digest = XOR_i shift(crc_i, hi - end_i).   crc32c.hip multiplies by x^K for compile-time K only (xmul<K>); here the power
// is a run-time byte count, so the multiplication is a general one: gfx950 has no carry-less multiply, it is 32 shift-and-xor steps.
// The selection of the rows and their checks are the indexed read's (frame_index_device.h); nothing of them is restated here.  DESIGN.md 4.22.
#pragma once
#include "frame_index_device.h"

namespace {

constexpr u32 kCrcPoly = 0x82F63B78u;
constexpr u32 kDigestRows = 64;             // R: interior rows per work item (one per lane of a wavefront)

// the inverse of crc32c_mask (snp_device.h)
__host__ __device__ __forceinline__ u32 crc_unmask(u32 m)
{
    const u32 r = m - 0xa282ead8u;
    return (r << 15) | (r >> 17);
}

// a * b mod P, reflected: bit 31 - i of a is the coefficient of x^i.  32 fixed steps, no branch on the data.
__host__ __device__ constexpr u32 gf2_mul(u32 a, u32 b)
{
    u32 p = 0;
    for (int i = 0; i < 32; ++i) {
        p ^= (a & (0x80000000u >> i)) ? b : 0u;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}

// x^(8 * 2^k) mod P for k = 0 .. 63: the powers a byte count's set bits select (x^8 reflected is 0x00800000; each entry is the square of the last)
struct CrcShiftTable {
    u32 t[64];
    constexpr CrcShiftTable() : t{}
    {
        u32 v = 0x00800000u;
        for (int k = 0; k < 64; ++k) {
            t[k] = v;
            v = gf2_mul(v, v);
        }
    }
};
inline constexpr CrcShiftTable kCrcShift{};

// c * x^(8n) mod P: the CRC register after n more zero bytes.  Every u64 n is legal (the table goes up to 2^63 bytes).
// On the device k is wave-uniform, so the table entry is a scalar constant load; lanes whose n lacks bit k sit the multiply out.
__host__ __device__ inline u32 crc_shift(u32 c, u64 n)
{
    for (u32 k = 0; n; ++k, n >>= 1)
        if (n & 1) c = gf2_mul(kCrcShift.t[k], c);
    return c;
}

// plain CRC of A || B from the plain CRCs of A and B and B's length
__host__ __device__ __forceinline__ u32 crc_combine(u32 crc_a, u32 crc_b, u64 len_b) { return crc_shift(crc_a, len_b) ^ crc_b; }

// One request against the index and the headers of its edge rows, as k_ix_plan of the indexed read plans it, with no capacity (ix_plan's `small`
// never arises).  status: what the plan answers (SNP_OK: planned).  hh, ht: the hops of the head and tail edge rows when k.head / k.last.
struct DgPlan {
    IxPlan k;
    Hop hh, ht;
    u64 interior;       // rows combined from their headers alone
};
__host__ __device__ inline DgPlan dg_plan(const FrameIndex& x, const u8* __restrict__ in, const u64* __restrict__ in_off, const u64* __restrict__ in_len,
                                          u32 nstreams, u32 b, u64 req_off, u64 req_len)
{
    DgPlan d{};
    d.k = ix_plan(x, nstreams, b, req_off, req_len, ~0ull);
    if (d.k.status != SNP_OK || d.k.r0 >= d.k.r1) return d;
    const u8* const p = in + in_off[b];
    const u64 n = in_len[b];
    const bool good = (!d.k.head || ix_row_check(x, p, n, d.k, d.k.r0, false, &d.hh)) && (!d.k.last || ix_row_check(x, p, n, d.k, d.k.r1 - 1, false, &d.ht));
    if (good) d.interior = d.k.interior();
    else d.k.status = SNP_ERR_BAD_ARG;
    return d;
}

// Interior row i of a planned request (stream bytes p, n): false = the row fails the read's check (the request is SNP_ERR_BAD_ARG).  *term = what
// the row adds to the digest: its header's CRC, unmasked, shifted over the hi - end bytes behind it.  A zero-length row adds nothing and its
// header CRC is not looked at.  The body is never read: A CORRUPT BODY IS NOT NOTICED.
__host__ __device__ inline bool dg_row_term(const FrameIndex& x, const u8* __restrict__ p, u64 n, const IxPlan& k, u64 i, u32* term)
{
    Hop h{};
    *term = 0;
    if (i >= k.f1 || !ix_row_check(x, p, n, k, i, true, &h)) return false;
    if (h.dec) *term = crc_shift(crc_unmask(h.crc), k.hi - ix_row_end(x, k.f1, k.total, i));
    return true;
}

// The part of an edge chunk [s, s + d) inside the window [lo, hi): [*from, *to), possibly empty (then *from == *to)
__host__ __device__ __forceinline__ void dg_edge_part(u64 s, u64 d, u64 lo, u64 hi, u64* from, u64* to)
{
    const u64 f = s > lo ? s : lo, t = s + d < hi ? s + d : hi;
    *from = f;
    *to = t > f ? t : f;
}

}  // namespace
