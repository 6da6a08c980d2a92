"""Inputs for the compressor tests: the fuzz generator, a tracer of the reference parse, and a directed set built with it.

Plain Python and numpy; imports nothing native (test_gpu_compress_matrix.py and the CPU tests share it).

  * EDGE_LENGTHS / make_block: the fuzz generator of test_gpu_fuzz.py.  The seeds recorded in profiles/*fuzz_log* refer to its
    sequences, so it must not change (test_compress_inputs.py pins a sha256 of them).
  * trace(fragment, variant) -> (tokens, events): the parse of oracle/pymodel.py::fragment, with a counter per EVENT CLASS -- the
    places where a kernel that follows the same parse takes another path (tag forms, the 16 / 32 / 64-byte pieces of literals and
    match extension, the fragment end, the skip heuristic, empty buckets, the probe after a copy, table-size boundaries).
  * directed(variant, seed) -> list[bytes]: for every class at least PER_CLASS fragments in which trace() shows the event.  A fragment
    is a planted template (incompressible filler, a repeat at a chosen distance, length and end position, a breaking byte, a tail);
    a candidate is kept only when the tracer confirms the event.

What the reference parse cannot produce (checked by test_compress_inputs.py, so the list below is arithmetic, not an omission):
  * a literal BEFORE A COPY has length ip - next_emit, where ip is a probe position of the scan that began at next_emit; the scan's
    offsets are fixed by the skip rule (1 .. 33, 35, 37 .. 65, 68 ..): 60, 64, 256 and 257 are not among them.  Literals of those
    lengths exist only as the remainder after the last copy; the classes lit_N count a literal of N bytes wherever it stands, and
    lit_before_copy_N exists for the reachable N.
  * a copy's offset is at most 65 519: the hit lies at ip <= n - 16 - (its stride) <= 65 520 and the candidate at >= 1 (position 0 is a
    candidate only through an empty bucket: offset = ip <= 65 520).  "Offset 65 535" cannot occur in a 64 KiB fragment; off_max is the
    class of offsets >= 65 500, built at 65 519 / 65 520.
"""
from __future__ import annotations

import functools
from collections import Counter

import numpy as np

from oracle import pymodel as P

EDGE_LENGTHS = [0, 1, 3, 4, 14, 15, 16, 17, 18, 19, 31, 32, 60, 61, 64, 65, 255, 256, 257, 4095, 4096, 16383, 16384, 16385,
                32768, 65520, 65521, 65535, 65536]


def make_block(rng: np.random.Generator, text: np.ndarray) -> np.ndarray:
    n = int(rng.choice(EDGE_LENGTHS)) if rng.integers(0, 3) == 0 else int(rng.integers(0, 65537))
    kind = int(rng.integers(0, 7))
    if kind == 0:                                             # incompressible
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == 1:                                             # text window with mutations
        s = int(rng.integers(0, len(text)))
        b = np.resize(np.roll(text, -s), n).copy()
        k = int(rng.integers(0, max(1, n // 20) + 1))
        if n and k:
            b[rng.integers(0, n, k)] = rng.integers(0, 256, k, dtype=np.uint8)
        return b
    if kind == 2:                                             # tiny alphabet: long matches, pattern copies
        return rng.integers(0, int(rng.integers(1, 4)), n, dtype=np.uint8)
    if kind == 3:                                             # runs of random length
        out = np.empty(n, dtype=np.uint8)
        pos = 0
        while pos < n:
            L = int(rng.integers(1, 1 << int(rng.integers(1, 11))))
            out[pos:pos + L] = rng.integers(0, 256)
            pos += L
        return out
    if kind == 4:                                             # random bytes with repeats copied from random distances
        out = rng.integers(0, 256, n, dtype=np.uint8)
        pos = 0
        while pos < n:
            pos += int(rng.integers(1, 200))
            if pos >= n:
                break
            dist = int(rng.integers(1, min(pos, 65535) + 1))
            L = min(int(rng.integers(4, 1 << int(rng.integers(3, 9)))), n - pos)
            for i in range(0, L, dist):                       # forward copy semantics (overlap allowed)
                out[pos + i: pos + min(i + dist, L)] = out[pos + i - dist: pos - dist + min(i + dist, L)]
            pos += L
        return out
    if kind == 5:                                             # periodic pattern with a defect now and then
        P = int(rng.integers(1, 70))
        b = np.resize(rng.integers(0, 256, P, dtype=np.uint8), n).copy()
        k = int(rng.integers(0, 6))
        if n and k:
            b[rng.integers(0, n, k)] ^= 0xFF
        return b
    a, c = make_block(rng, text), make_block(rng, text)       # two halves of different kinds
    return np.concatenate([a[: len(a) // 2], c[: len(c) // 2]])[:65536]


# ---------------------------------------------------------------------------------------------------------------- event classes

COPY_LENGTHS = [4, 11, 12, 15, 16, 17, 31, 32, 33, 48, 59, 60, 61, 64, 65, 66, 67, 68, 69, 127, 128, 131, 132]
LITERAL_LENGTHS = [1, 14, 15, 16, 17, 60, 61, 64, 65, 256, 257]
FRAGMENT_LENGTHS = [15, 16, 30, 31, 32, 33, 47] + [v for k in range(8, 15) for v in (1 << k, (1 << k) + 1)]   # + each table-size boundary
HIT_PROBES = [31, 32, 33, 34]


def scan_offsets(upto: int) -> list[int]:
    """ip - next_emit of the successive probes of one scan (pymodel.fragment: skip = 32, step = skip >> 5, skip += step)."""
    out, skip, off = [], 32, 1
    while off <= upto:
        out.append(off)
        step = skip >> 5
        skip += step
        off += step
    return out


_SCAN = scan_offsets(65536)
_SCAN_SET = set(_SCAN)
LITERALS_BEFORE_COPY = [v for v in LITERAL_LENGTHS if v in _SCAN_SET]            # 1 14 15 16 17 61 65

CLASSES = (
    [f"copy_len_{v}" for v in COPY_LENGTHS] + ["copy_len_ge4096"]
    + ["off2047_len_lt12", "off2048_len_lt12", "off_lt2048_len_ge12"]
    + ["off_1", "off_2", "off_3", "off_ge65000", "off_max"]
    + [f"lit_{v}" for v in LITERAL_LENGTHS] + [f"lit_before_copy_{v}" for v in LITERALS_BEFORE_COPY]
    + ["lit_whole_fragment", "lit_ge16_staged"]
    + ["end_limit_m1", "end_limit", "end_limit_p1", "end_n"]
    + ["base48_n_m1", "base48_n", "base48_n_p1"]
    + ["last_compare_8_at_n", "last_compare_byte_loop"]
    + ["scan_next_eq_limit", "scan_next_eq_limit_p1", "unrolled_skipped"]
    + [f"hit_probe_{v}" for v in HIT_PROBES] + ["hit_probe_ge64"]
    + ["empty_hit", "empty_near_miss"]
    + ["post_hit", "post_chain_ge130", "post_miss", "post_bucket_m1_diff", "post_bucket_m1_equal"]
    + [f"n_{v}" for v in FRAGMENT_LENGTHS]
    + ["check_collision", "pair_same_bucket_equal", "pair_same_bucket_diff"]
)
PER_CLASS = 3


def check_bits(d: int) -> int:
    """KERNEL-AWARE: the 16 check bits the lane kernel keeps beside a table position (compress_lanes.hip:41, check_bits).  The reference
    has no such thing; the classes check_collision and pair_same_bucket_* exist because of it."""
    return (d * 0x9E3779B1) & 0xFFFF0000


def trace(f, variant: int):
    """-> (tokens, events).  tokens: ("lit", start, length) / ("copy", offset, length) in order (encode() turns them into the stream);
    events: Counter over CLASSES.  The control flow is pymodel.fragment's, statement for statement."""
    f = bytes(f)
    n = len(f)
    ev: Counter = Counter()
    tokens: list = []
    if n in FRAGMENT_LENGTHS:
        ev[f"n_{n}"] += 1
    H = P.h_crc if variant == P.HASH_CRC32C else P.h_mul
    ld32 = lambda p: int.from_bytes(f[p:p + 4], "little")   # noqa: E731
    ts = P.tsize(n)
    mask = 2 * (ts - 1)
    table = [0] * ts
    first4 = ld32(0)
    # the output position, and what the lane kernel's staged-output form (compress_lanes.hip, kOptStagedOutput) holds in LDS at that moment:
    # bytes [flushed, op); whole 64-byte runs leave as they fill, a literal of >= 16 bytes drains the stage and goes around it
    pos = {"op": len(P.varint32(n)), "flushed": len(P.varint32(n))}

    def advance(k):
        pos["op"] += k
        while pos["op"] - pos["flushed"] >= 64:
            pos["flushed"] += 64

    def lit(s, l, before_copy):
        tokens.append(("lit", s, l))
        if l in LITERAL_LENGTHS:
            ev[f"lit_{l}"] += 1
            if before_copy:
                ev[f"lit_before_copy_{l}"] += 1
        if before_copy and l >= 16:
            if 1 <= pos["op"] - pos["flushed"] <= 63:
                ev["lit_ge16_staged"] += 1
            pos["op"] += l + (1 if l <= 60 else 2 if l <= 256 else 3)
            pos["flushed"] = pos["op"]
        else:
            advance(l + (1 if l <= 60 else 2 if l <= 256 else 3))

    def copy(base, cand, m):
        off = base - cand
        tokens.append(("copy", off, m))
        if m in COPY_LENGTHS:
            ev[f"copy_len_{m}"] += 1
        if m >= 4096:
            ev["copy_len_ge4096"] += 1
        if m < 12 and off == 2047:
            ev["off2047_len_lt12"] += 1
        if m < 12 and off == 2048:
            ev["off2048_len_lt12"] += 1
        if m >= 12 and off < 2048:
            ev["off_lt2048_len_ge12"] += 1
        if off <= 3:
            ev[f"off_{off}"] += 1
        if off >= 65000:
            ev["off_ge65000"] += 1
        if off >= 65500:
            ev["off_max"] += 1
        end = base + m
        for name, v in (("end_limit_m1", n - 16), ("end_limit", n - 15), ("end_limit_p1", n - 14), ("end_n", n)):
            if end == v:
                ev[name] += 1
        if m >= 16:                                           # the first 32-byte extension step starts at base + 16
            for name, v in (("base48_n_m1", n - 1), ("base48_n", n), ("base48_n_p1", n + 1)):
                if base + 48 == v:
                    ev[name] += 1
        s2, e = base + 4, m - 4                               # FindMatchLength(cand + 4, base + 4, n): 8-byte steps, then a byte loop
        q, r = divmod(n - s2, 8)
        if q >= 1 and r == 0 and e >= 8 * (q - 1):
            ev["last_compare_8_at_n"] += 1
        if r != 0 and e >= 8 * q:
            ev["last_compare_byte_loop"] += 1
        k, l = 0, m                                           # the tags of pymodel._copy
        if l < 12:
            k = 2 if off < 2048 else 3
        else:
            while l >= 68:
                k, l = k + 3, l - 64
            if l > 64:
                k, l = k + 3, l - 60
            k += 3
        advance(k)

    def probe_events(d, c):
        if c == 0:                                            # an empty bucket (position 0 is never inserted)
            x = d ^ first4
            if x and sum(1 for s in (0, 8, 16, 24) if (x >> s) & 255) == 1:
                ev["empty_near_miss"] += 1
        else:
            dc = ld32(c)
            if dc != d and check_bits(dc) == check_bits(d):   # KERNEL-AWARE (check_bits above): the kernel has to fetch the bytes to see the miss
                ev["check_collision"] += 1

    ip = 0
    if n >= 15:
        limit = n - 15
        while True:                                           # OUTER
            next_emit = ip
            ip += 1
            skip = 32
            found = False
            cand = 0
            nprobe = 0
            prev = None                                       # (position, bucket, dword) of the scan's previous probe

            def scan_probe(p, d):
                nonlocal prev
                h = H(d, mask)
                c = table[h]
                # KERNEL-AWARE: with two probes per trip the second one takes the first one's entry from a register when both fall into one bucket
                if prev is not None and prev[0] + 1 == p and prev[1] == h:
                    ev["pair_same_bucket_equal" if prev[2] == d else "pair_same_bucket_diff"] += 1
                prev = (p, h, d)
                probe_events(d, c)
                table[h] = p
                return c

            if limit - ip >= 16:
                for j in range(16):
                    p = ip + j
                    d = ld32(p)
                    nprobe += 1
                    c = scan_probe(p, d)
                    if ld32(c) == d:
                        ip, cand, found = p, c, True
                        break
                if not found:
                    ip += 16
                    skip += 16
            else:
                ev["unrolled_skipped"] += 1
            remainder = False
            if not found:
                while True:
                    d = ld32(ip)
                    bb = skip >> 5
                    skip += bb
                    nxt = ip + bb
                    if nxt > limit:
                        if nxt == limit + 1:
                            ev["scan_next_eq_limit_p1"] += 1
                        ip = next_emit
                        remainder = True
                        break
                    if nxt == limit:
                        ev["scan_next_eq_limit"] += 1
                    nprobe += 1
                    c = scan_probe(ip, d)
                    if ld32(c) == d:
                        cand = c
                        break
                    ip = nxt
            if remainder:
                break
            if nprobe in HIT_PROBES:
                ev[f"hit_probe_{nprobe}"] += 1
            if nprobe >= 64:
                ev["hit_probe_ge64"] += 1
            if cand == 0:
                ev["empty_hit"] += 1
            lit(next_emit, ip - next_emit, True)
            chain = 0
            while True:                                       # repeat ... until ld32(cand) != d
                base = ip
                m = 4
                while ip + m < n and f[cand + m] == f[ip + m]:
                    m += 1
                ip += m
                copy(base, cand, m)
                if ip >= limit:
                    remainder = True
                    break
                dm1 = ld32(ip - 1)
                hm1 = H(dm1, mask)
                table[hm1] = ip - 1
                d = ld32(ip)
                h = H(d, mask)
                if h == hm1:
                    ev["post_bucket_m1_equal" if d == dm1 else "post_bucket_m1_diff"] += 1
                cand = table[h]
                probe_events(d, cand)
                table[h] = ip
                if ld32(cand) != d:
                    ev["post_miss"] += 1
                    break
                ev["post_hit"] += 1
                chain += 1
                if chain == 130:
                    ev["post_chain_ge130"] += 1
            if remainder:
                break
    if ip < n:
        lit(ip, n - ip, False)
    if n >= 15 and len(tokens) == 1:
        ev["lit_whole_fragment"] += 1
    return tokens, ev


def encode(f, tokens) -> bytes:
    """The block the tokens stand for (preamble + pymodel's _literal / _copy): what O.compress gives for a fragment of <= 64 KiB."""
    f = bytes(f)
    out = bytearray(P.varint32(len(f)))
    for kind, a, l in tokens:
        if kind == "lit":
            P._literal(out, f, a, l)
        else:
            P._copy(out, a, l)
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------- directed set

def _filler(rng, n) -> bytearray:
    return bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())


def _plant(buf: bytearray, src: int, dst: int, length: int) -> int:
    """A repeat of buf[src:] at dst (forward-copy semantics: dst - src may be shorter than the length), a differing byte in front of it
    and a breaking byte behind it.  -> the position behind the repeat."""
    n = len(buf)
    length = min(length, n - dst)
    if src >= 1 and buf[dst - 1] == buf[src - 1]:
        buf[dst - 1] ^= 0x5A
    for i in range(length):
        buf[dst + i] = buf[src + i]
    end = dst + length
    if end < n and buf[end] == buf[src + length]:
        buf[end] ^= 0xFF
    return end


def _ri(rng, lo, hi) -> int:                                  # lo .. hi inclusive
    return int(rng.integers(lo, hi + 1))


def _near(rng, length, dist=None, tail=None, src=None) -> bytearray:
    """One repeat inside the stride-1 zone of the fragment's first scan: candidate at 1 .. 8, hit at <= 32."""
    src = _ri(rng, 1, 8) if src is None else src
    dist = _ri(rng, 4, 20) if dist is None else dist
    tail = _ri(rng, 16, 40) if tail is None else tail
    dst = src + dist
    buf = _filler(rng, dst + length + tail)
    _plant(buf, src, dst, length)
    return buf


def _two(rng, gap, len2=None, tail=None, len1=None) -> bytearray:
    """Two repeats: the second one `gap` bytes behind the end of the first (gap 0: the probe after the copy hits), its candidate in the
    stride-1 zone in front of the first."""
    src1, d1 = _ri(rng, 6, 10), _ri(rng, 6, 14)
    dst1 = src1 + d1
    len1 = _ri(rng, 4, 30) if len1 is None else len1
    len2 = _ri(rng, 4, 14) if len2 is None else len2
    tail = _ri(rng, 16, 40) if tail is None else tail
    dst2 = dst1 + len1 + gap
    buf = _filler(rng, dst2 + len2 + tail)
    _plant(buf, src1, dst1, len1)
    _plant(buf, _ri(rng, 1, src1 - 5), dst2, len2)             # bytes 1 .. src1 - 1 + 4 lie in front of the first repeat's source
    return buf


def _far(rng, n, src, dst, length) -> bytearray | None:
    """A repeat at a distance beyond the stride-1 zone.  The skip heuristic probes an incompressible stretch at strides that grow with its
    length (step = (distance from the scan's start + 32) / 32), so `dst` is reached over a ladder: 6-byte repeats of the bytes at 2 .. 7,
    each of which ends a scan and starts the next one with stride 1 -- the first inside the first scan's stride-1 zone, each further one at
    a probe position of the scan its predecessor started, the last one 2 .. 32 bytes in front of `dst`.  `src` < 17 lies in front of the first
    rung.  None: the fragment has no room for the strides."""
    limit = n - 15
    buf = _filler(rng, n)
    pos = _ri(rng, max(src + 5, 12), 26)
    while True:
        _plant(buf, 2, pos, 6)
        e = pos + 6
        rem = dst - e
        if 2 <= rem <= 32:
            break
        g = next((g for g in reversed(_SCAN) if g <= min(rem - 8, 32 * (limit - e)) and e + g + ((g + 32) >> 5) <= limit), None)
        if g is None or rem < 2:
            return None
        pos = e + g
    _plant(buf, src, dst, length)
    return buf


def _np_hash(d: np.ndarray, mask: int, variant: int) -> np.ndarray:
    d = d.astype(np.uint64)
    if variant == P.HASH_CRC32C:
        P._step32_fast(0)
        t = [np.array(P._STEP8[k], dtype=np.uint64) for k in range(4)]
        x = (d ^ np.uint64(mask)).astype(np.int64)
        v = t[0][x & 255] ^ t[1][(x >> 8) & 255] ^ t[2][(x >> 16) & 255] ^ t[3][x >> 24]
    else:
        v = ((d * np.uint64(0x1E35A7BD)) & np.uint64(0xFFFFFFFF)) >> 17
    return (v & np.uint64(mask)) >> 1


@functools.lru_cache(maxsize=None)
def _collision_pairs(variant: int, seed: int):
    """Pairs of different dwords with the same bucket of a 256-entry table AND the same check bits: 24 bits in all, so 20 000 random dwords
    hold about a dozen pairs (sorted search)."""
    rng = np.random.default_rng([seed, variant, 24])
    d = rng.integers(0, 1 << 32, 20000, dtype=np.uint64)
    key = (_np_hash(d, 2 * 255, variant) << 16) | (((d * np.uint64(0x9E3779B1)) & np.uint64(0xFFFF0000)) >> 16)
    order = np.argsort(key, kind="stable")
    ks, ds = key[order], d[order]
    at = np.nonzero((ks[1:] == ks[:-1]) & (ds[1:] != ds[:-1]))[0]
    return [(int(ds[i]), int(ds[i + 1])) for i in at]


def _five_in_one_bucket(rng, variant, mask, b0=None) -> bytes | None:
    """Five bytes whose two dwords (at +0 and +1) differ and fall into one bucket."""
    for _ in range(64):
        head = bytes([_ri(rng, 0, 255) if b0 is None else b0]) + bytes(_ri(rng, 0, 255) for _ in range(3))
        d1 = int.from_bytes(head, "little")
        d2 = (d1 >> 8) | (np.arange(256, dtype=np.uint64) << 24)
        ok = np.nonzero((_np_hash(d2, mask, variant) == _np_hash(np.array([d1]), mask, variant)[0]) & (d2 != d1))[0]
        if ok.size:
            return head + bytes([int(ok[_ri(rng, 0, ok.size - 1)])])
    return None


def _recipes(variant: int, seed: int):
    """class -> function(rng) -> candidate fragment (or None).  The tracer decides whether a candidate is kept."""
    R = {}
    for v in COPY_LENGTHS:
        R[f"copy_len_{v}"] = lambda rng, v=v: _near(rng, v)
    R["copy_len_ge4096"] = lambda rng: _near(rng, 4096 + _ri(rng, 0, 300))
    for off in (2047, 2048):
        R[f"off{off}_len_lt12"] = lambda rng, off=off: (lambda s: _far(rng, s + off + _ri(rng, 40, 200), s, s + off, _ri(rng, 4, 11)))(_ri(rng, 9, 16))
    R["off_lt2048_len_ge12"] = lambda rng: _near(rng, _ri(rng, 12, 40))
    for off in (1, 2, 3):
        R[f"off_{off}"] = lambda rng, off=off: _near(rng, _ri(rng, 6, 24), dist=off)
    R["off_ge65000"] = lambda rng: (lambda s: _far(rng, 65536 - _ri(rng, 0, 40), s, s + _ri(rng, 65000, 65400), _ri(rng, 4, 40)))(_ri(rng, 9, 16))

    def off_max(rng):
        # n = 65 536, limit = 65 521: the last position a scan probes is 65 520 (with stride 1).  Candidate at 1: offset 65 519.
        return _far(rng, 65536, 1, 65520, _ri(rng, 4, 16))
    R["off_max"] = off_max

    for v in LITERAL_LENGTHS:                                  # as the remainder behind the only copy (every length is possible there)
        R[f"lit_{v}"] = lambda rng, v=v: _near(rng, _ri(rng, 4, 40), tail=v)
    for v in LITERALS_BEFORE_COPY:
        R[f"lit_before_copy_{v}"] = lambda rng, v=v: _two(rng, v)
    R["lit_whole_fragment"] = lambda rng: _filler(rng, _ri(rng, 15, 400))
    R["lit_ge16_staged"] = lambda rng: _two(rng, _ri(rng, 16, 33))
    for name, tail in (("end_limit_m1", 16), ("end_limit", 15), ("end_limit_p1", 14), ("end_n", 0)):
        R[name] = lambda rng, tail=tail: _near(rng, _ri(rng, 4, 80), tail=tail)
    for name, delta in (("base48_n_m1", -1), ("base48_n", 0), ("base48_n_p1", 1)):
        def base48(rng, delta=delta):                          # n = base + 48 - delta; the match is 16 .. n - base bytes long
            length = _ri(rng, 16, 48 - delta)
            return _near(rng, length, tail=48 - delta - length)
        R[name] = base48
    R["last_compare_8_at_n"] = lambda rng: _near(rng, 4 + 8 * _ri(rng, 1, 9), tail=0)
    R["last_compare_byte_loop"] = lambda rng: _near(rng, 4 + 8 * _ri(rng, 0, 9) + _ri(rng, 1, 7), tail=0)
    R["scan_next_eq_limit"] = lambda rng: _filler(rng, _ri(rng, 16, 300))
    R["scan_next_eq_limit_p1"] = lambda rng: _filler(rng, _ri(rng, 16, 300))
    R["unrolled_skipped"] = lambda rng: _filler(rng, _ri(rng, 15, 31)) if _ri(rng, 0, 1) else _near(rng, _ri(rng, 4, 20), tail=_ri(rng, 17, 30))
    for v in HIT_PROBES + [64]:
        def hit_probe(rng, v=v):
            k = v if v < 64 else _ri(rng, 64, 90)
            src = _ri(rng, 1, 10)
            buf = _filler(rng, _SCAN[k - 1] + 60)
            _plant(buf, src, _SCAN[k - 1], _ri(rng, 4, 20))
            return buf
        R[f"hit_probe_{v}" if v < 64 else "hit_probe_ge64"] = hit_probe

    def empty(rng, near_miss):
        buf = _filler(rng, _ri(rng, 40, 200))
        dst = _ri(rng, 5, 30)
        buf[dst:dst + 4] = buf[0:4]
        if buf[dst + 4] == buf[4]:
            buf[dst + 4] ^= 0xFF
        if near_miss:                                          # the same dword probes the same empty bucket; the fragment starts with other bytes
            buf[0] ^= 1 << _ri(rng, 0, 7)
        return buf
    R["empty_hit"] = lambda rng: empty(rng, False)
    R["empty_near_miss"] = lambda rng: empty(rng, True)
    R["post_hit"] = lambda rng: _two(rng, 0)
    R["post_chain_ge130"] = lambda rng: bytearray(rng.integers(0, 2, _ri(rng, 2500, 4000), dtype=np.uint8).tobytes())
    R["post_miss"] = lambda rng: _near(rng, _ri(rng, 4, 40))

    def post_m1(rng, equal):
        length = _ri(rng, 4, 30)
        src, dist = _ri(rng, 1, 8), _ri(rng, 6, 20)
        end = src + dist + length
        buf = _filler(rng, end + _ri(rng, 20, 60))
        _plant(buf, src, src + dist, length)
        if equal:
            buf[end:end + 4] = bytes([buf[end - 1]]) * 4       # dword(ip - 1) == dword(ip): a run begins in the copy's last byte
        else:
            five = _five_in_one_bucket(rng, variant, 2 * (P.tsize(len(buf)) - 1), buf[end - 1])
            if five is None:
                return None
            buf[end:end + 4] = five[1:]
        return buf
    R["post_bucket_m1_equal"] = lambda rng: post_m1(rng, True)
    R["post_bucket_m1_diff"] = lambda rng: post_m1(rng, False)

    for v in FRAGMENT_LENGTHS:
        def length_case(rng, v=v):
            kind = _ri(rng, 0, 2)
            if kind == 0:
                return _filler(rng, v)
            if kind == 1:
                return bytearray(rng.integers(0, 3, v, dtype=np.uint8).tobytes())
            buf = _filler(rng, v)                              # a repeat that runs into the fragment's end
            dst = _ri(rng, 6, max(6, min(30, v - 5)))
            _plant(buf, _ri(rng, 1, dst - 4), dst, v)
            return buf
        R[f"n_{v}"] = length_case

    def collision(rng):
        pairs = _collision_pairs(variant, seed)
        if not pairs:
            return None
        a, b = pairs[_ri(rng, 0, len(pairs) - 1)]
        buf = _filler(rng, _ri(rng, 60, 256))                  # <= 256 bytes: the 256-entry table the pairs were searched for
        src = _ri(rng, 1, 12)
        dst = src + _ri(rng, 4, 16)
        buf[src:src + 4] = a.to_bytes(4, "little")
        buf[dst:dst + 4] = b.to_bytes(4, "little")
        return buf
    R["check_collision"] = collision

    def pair(rng, equal):
        buf = _filler(rng, _ri(rng, 60, 256))
        p = _ri(rng, 3, 25)
        if equal:
            buf[p:p + 5] = bytes([buf[p]]) * 5
            if buf[p - 1] == buf[p]:
                buf[p - 1] ^= 0xFF
        else:
            five = _five_in_one_bucket(rng, variant, 2 * 255)
            if five is None:
                return None
            buf[p:p + 5] = five
        return buf
    R["pair_same_bucket_equal"] = lambda rng: pair(rng, True)
    R["pair_same_bucket_diff"] = lambda rng: pair(rng, False)
    return R


# Fragments a test run once reduced a failure to, kept by name: (name, variant or None for both, bytes).
NAMED_CASES: list[tuple[str, int | None, bytes]] = []

ATTEMPTS = 400


@functools.lru_cache(maxsize=None)
def directed_named(variant: int, seed: int = 0) -> tuple[tuple[str, bytes], ...]:
    """((class, fragment), ...): PER_CLASS fragments for every class of CLASSES, each confirmed by trace(); then NAMED_CASES."""
    recipes = _recipes(variant, seed)
    assert set(recipes) == set(CLASSES)
    out = []
    for ci, name in enumerate(CLASSES):
        rng = np.random.default_rng([seed, variant, ci])
        found: list[bytes] = []
        for _ in range(ATTEMPTS):
            cand = recipes[name](rng)
            if cand is None:
                continue
            cand = bytes(cand)
            if cand not in found and trace(cand, variant)[1][name] > 0:
                found.append(cand)
                if len(found) == PER_CLASS:
                    break
        assert len(found) == PER_CLASS, f"directed(): class {name} (hash {variant}): {len(found)} of {PER_CLASS} fragments in {ATTEMPTS} attempts"
        out += [(name, b) for b in found]
    out += [(name, b) for name, v, b in NAMED_CASES if v is None or v == variant]
    return tuple(out)


def directed(variant: int, seed: int = 0) -> list[bytes]:
    return [b for _name, b in directed_named(variant, seed)]


def _trace_job(job):
    f, variant = job
    tokens, ev = trace(f, variant)
    return encode(f, tokens), [k for k, v in ev.items() if v]


def trace_all(fragments, variant: int, workers: int = 1):
    """-> (the tracer's encoding of every fragment, census: class -> number of FRAGMENTS in which the event occurs).  The parse is a pure-Python
    loop, so a large set is spread over `workers` processes."""
    jobs = [(bytes(f), variant) for f in fragments]
    if workers > 1 and len(jobs) > 64:
        import multiprocessing
        with multiprocessing.get_context("fork").Pool(workers) as pool:
            done = pool.map(_trace_job, jobs, chunksize=8)
    else:
        done = [_trace_job(j) for j in jobs]
    total: Counter = Counter()
    for _enc, names in done:
        total.update(names)
    return [enc for enc, _names in done], {k: int(total[k]) for k in CLASSES}
