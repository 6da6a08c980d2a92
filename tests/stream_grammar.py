"""Legal Snappy block streams drawn from the whole tag grammar, not from the dialect a 64 KiB-fragment compressor emits -- TEST INFRASTRUCTURE
ONLY, plain Python, no GPU.  The block decoders keep separate code for forms our own compressor and the oracle's never write: copy-4, offsets of
65536 and more, literals whose length field is longer than it has to be, copy-1 / copy-2 where a shorter form would do, 65..128-byte literals
written with 2..4 length bytes.  build() emits such streams tag by tag and constructs the output itself while it does (copies byte by byte): a
third statement of the semantics next to oracle/snappy_oracle.c and oracle/pymodel.py.  mutate() makes near-misses that know where the tags
are; framed() wraps streams as the compressed chunks of a Snappy framed stream.  tests/test_stream_grammar.py holds the generator to the oracle
and to its own coverage claims; tests/test_gpu_stream_grammar.py runs the device decoders on what it gives."""
import random

import frame_buffers_model as FM
import oracle as O

B = 65536
PROFILES = ("uniform", "copy4", "fat-literals", "two-slot", "pattern", "dense", "far")
LITERAL_EDGES = (1, 2, 3, 59, 60, 61, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257)
COPY_LENGTH_EDGES = (1, 2, 3, 4, 5, 11, 12, 16, 17, 32, 63, 64)
OFFSET_EDGES = tuple(range(1, 18)) + (63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 2047, 2048, 4095, 65535, 65536, 65537)
TAG_LIKE = (0xF0, 0xF4, 0xFC, 0xFF, 0x14)        # as tags: literals with 1, 2 and 4 length bytes, a copy-4 of 64, a literal of 6
LIT, COPY = "lit", "copy"


def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def min_literal_form(n: int) -> int:
    """The fewest length bytes (0..4) a literal of n bytes can be written with."""
    return 0 if n <= 60 else ((n - 1).bit_length() + 7) // 8


def literal_header(n: int, form: int) -> bytes:
    assert n >= 1 and min_literal_form(n) <= form <= 4
    if form == 0:
        return bytes([(n - 1) << 2])
    return bytes([(59 + form) << 2]) + (n - 1).to_bytes(form, "little")


def copy_forms(length: int, offset: int):
    """The copy types (1 / 2 / 4) that can hold (length, offset)."""
    forms = [4]
    if offset < 65536:
        forms.append(2)
        if 4 <= length <= 11 and offset < 2048:
            forms.append(1)
    return forms


def copy_tag(length: int, offset: int, form: int) -> bytes:
    assert 1 <= length <= 64 and 0 <= offset <= 0xFFFFFFFF
    if form == 1:
        assert 4 <= length <= 11 and offset < 2048
        return bytes([1 | ((length - 4) << 2) | ((offset >> 8) << 5), offset & 255])
    if form == 2:
        assert offset < 65536
        return bytes([2 | ((length - 1) << 2)]) + offset.to_bytes(2, "little")
    return bytes([3 | ((length - 1) << 2)]) + offset.to_bytes(4, "little")


class _Emitter:
    def __init__(self, rnd, total, fragment_local, bounded):
        self.rnd, self.total, self.fragment_local, self.bounded = rnd, total, fragment_local, bounded
        self.out = bytearray(varint(total))
        self.raw = bytearray()
        self.tags = []
        # bounded: len(stream) - total may reach 38 + total // 6; every fragment still to come may end in a literal with a 5-byte header
        self.allowance = 38 + total // 6

    def room(self) -> int:
        """Output bytes the next tag may produce."""
        rem = self.total - len(self.raw)
        if self.fragment_local:
            rem = min(rem, B - len(self.raw) % B)
        return rem

    def reach(self) -> int:
        """The largest offset a copy may use now (0: only a literal can come)."""
        return len(self.raw) % B if self.fragment_local else len(self.raw)

    def affordable(self, tag_bytes: int, produces: int) -> bool:
        if not self.bounded:
            return True
        left = self.total - len(self.raw) - produces
        reserve = 5 * ((left + B - 1) // B + 1)
        return len(self.out) + tag_bytes - (len(self.raw) + produces) + reserve <= self.allowance

    def saver(self):
        """bounded, and the tag asked for would go over the bound: a 64-byte copy-2 (61 bytes gained), or -- nothing to copy from, a short
        tail -- one minimal literal to the end of the fragment, which the reserve of affordable() has paid for."""
        room, reach = self.room(), self.reach()
        if reach > 0 and room >= 64:
            return self.copy(64, min(reach, self.rnd.choice((1, 5, 64, 65, 700, 2048, 40000))), 2)
        n = room
        self.tags.append((len(self.out), len(self.raw), LIT, min_literal_form(n), n, 0))
        body = self.rnd.randbytes(n)
        self.out += literal_header(n, min_literal_form(n)) + body
        self.raw += body

    def literal(self, n: int, form: int, body: bytes):
        head = literal_header(n, form)
        if not self.affordable(len(head) + n, n):
            form = min_literal_form(n)
            head = literal_header(n, form)
            if not self.affordable(len(head) + n, n):
                return self.saver()
        self.tags.append((len(self.out), len(self.raw), LIT, form, n, 0))
        self.out += head
        self.out += body
        self.raw += body

    def copy(self, n: int, offset: int, form: int):
        if not self.affordable((2, 3, 5)[(1, 2, 4).index(form)], n):
            return self.saver()
        self.tags.append((len(self.out), len(self.raw), COPY, form, n, offset))
        self.out += copy_tag(n, offset, form)
        raw = self.raw
        for _ in range(n):                                   # byte by byte: a source that overlaps the destination repeats its pattern
            raw.append(raw[-offset])


def _body(rnd, n: int) -> bytes:
    how = rnd.random()
    if how < 0.2:
        return bytes(rnd.choice(TAG_LIKE) for _ in range(n)) if n < 200 else bytes([rnd.choice(TAG_LIKE)]) * n
    if how < 0.4:
        return bytes(rnd.choice(b"ab \n") for _ in range(n)) if n < 200 else (rnd.randbytes(7) * (n // 7 + 1))[:n]
    return rnd.randbytes(n)


def _literal_length(rnd, short: bool = False) -> int:
    how = rnd.random()
    if short:
        return rnd.choice((1, 1, 2, 3, 4, 7))
    if how < 0.5:
        return rnd.choice(LITERAL_EDGES)
    if how < 0.9:
        return rnd.randint(1, 70)
    return rnd.randint(1, 5000)


def _copy_length(rnd) -> int:
    return rnd.choice(COPY_LENGTH_EDGES) if rnd.random() < 0.5 else rnd.randint(1, 64)


def _copy_offset(rnd, produced: int, reach: int) -> int:
    how = rnd.random()
    if how < 0.5:
        off = rnd.choice(OFFSET_EDGES)
    elif how < 0.6:
        off = produced
    elif how < 0.8:
        off = rnd.randint(1, min(reach, 300))
    else:
        off = rnd.randint(1, reach)
    return min(off, reach)


def build(seed: int, total: int, profile: str, *, fragment_local: bool = False, bounded: bool = False):
    """-> (stream, raw, tags): a well-formed stream of exactly `total` output bytes, the bytes it decodes to, and one tuple per tag
    (ip, op, kind, form, length, offset) -- form = the number of literal length bytes (0..4) or the copy type (1 / 2 / 4).
    fragment_local: no tag's output crosses a multiple of 65536 and no copy reads from before the multiple of 65536 at or below its destination.
    bounded: len(stream) <= 38 + total + total // 6."""
    assert profile in PROFILES and 0 <= total < (1 << 31)
    rnd = random.Random(f"{profile}/{seed}/{total}/{int(fragment_local)}/{int(bounded)}")
    e = _Emitter(rnd, total, fragment_local, bounded)
    run_left, fat_k = 0, 0                                   # two-slot: short tags still to come before the next 65..128-byte literal
    while len(e.raw) < total:
        room, reach = e.room(), e.reach()
        produced = len(e.raw)
        want_copy, n, form, off = False, 0, None, 0
        if profile == "two-slot":
            if run_left == 0 and room >= 65:
                n = min(room, rnd.choice((65, 66, 96, 127, 128, rnd.randint(65, 128))))
                form = 1 + fat_k % 4
                fat_k += 1
                # the next one: a random number of short tags away, and every fourth time exactly on the last slot of a batch of 64
                at = len(e.tags) + 1
                run_left = (63 - at) % 64 + (64 if rnd.random() < 0.5 else 0) if fat_k % 4 == 0 else rnd.randint(0, 140)
            else:
                run_left = max(0, run_left - 1)
                want_copy = reach > 0 and rnd.random() < 0.6
                n = rnd.choice((1, 2, 3, 4, 5, 8, 11)) if want_copy else rnd.choice((1, 1, 2, 3))
                if want_copy:
                    off = _copy_offset(rnd, produced, reach)
                    n = min(n, room)
                    form = 4 if rnd.random() < 0.4 else rnd.choice(copy_forms(n, off))
        elif profile == "pattern":
            want_copy = reach > 0 and rnd.random() < 0.75
            if want_copy:
                off = min(rnd.randint(1, 16), reach)
                n = rnd.randint(off + 1, 64)
            else:
                n = _literal_length(rnd, short=True)
        elif profile == "dense":
            want_copy = reach > 0 and rnd.random() < 0.6
            n = rnd.randint(1, 3)
            form = 4
            if want_copy:
                off = _copy_offset(rnd, produced, reach)
        elif profile == "copy4":
            want_copy = reach > 0 and rnd.random() < 0.85
            if want_copy:
                n, off, form = _copy_length(rnd), _copy_offset(rnd, produced, reach), 4
            else:
                n = _literal_length(rnd, short=rnd.random() < 0.7)
        elif profile == "far" and produced >= B and not fragment_local and rnd.random() < 0.5:
            want_copy = True
            n = _copy_length(rnd)
            off = rnd.choice((B, B + 1, produced, rnd.randint(B, produced), rnd.randint(B, produced)))
            off = min(off, produced)
        else:                                                # uniform, fat-literals, and far below 65536
            want_copy = reach > 0 and rnd.random() < 0.6
            if want_copy:
                n, off = _copy_length(rnd), _copy_offset(rnd, produced, reach)
            else:
                n = _literal_length(rnd)
        n = min(n, room)
        if want_copy:
            if form is None:
                form = rnd.choice(copy_forms(n, off))
            elif form not in copy_forms(n, off):
                form = 4
            e.copy(n, off, form)
        else:
            low = min_literal_form(n)
            if form is None:
                form = rnd.randint(min(low + 1, 4), 4) if profile == "fat-literals" else rnd.randint(low, 4)
            e.literal(n, max(form, low), _body(rnd, n))
    stream, raw = bytes(e.out), bytes(e.raw)
    assert len(raw) == total and (not bounded or len(stream) <= 38 + total + total // 6)
    return stream, raw, e.tags


def preamble_bytes(stream: bytes) -> int:
    hb = 1
    while stream[hb - 1] & 0x80:
        hb += 1
    return hb


def is_fragment_local(tags) -> bool:
    return all(op // B == (op + n - 1) // B and (kind == LIT or off <= op % B) for _ip, op, kind, _f, n, off in tags)


# ---- near-misses ---------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("offset-past", "offset-zero", "offset-ffffffff", "offset-80000000", "offset-at-start", "last-length+1", "declared+1", "declared-1",
             "cut-trailer", "cut-body", "cut-after-tag", "extra-tag", "literal-7fffffff", "literal-80000000", "literal-ffffffff")
_TRAILER = {(LIT, 0): 0, (LIT, 1): 1, (LIT, 2): 2, (LIT, 3): 3, (LIT, 4): 4, (COPY, 1): 1, (COPY, 2): 2, (COPY, 4): 4}
_OFFSET_LIMIT = {1: 2048, 2: 65536, 4: 1 << 32}


def _pick(tags, fits):
    """The tag a mutation touches: the one nearest the middle of the stream that it fits (None: it fits none)."""
    mid = len(tags) // 2
    for d in range(len(tags)):
        for i in (mid + d, mid - d - 1):
            if 0 <= i < len(tags) and fits(tags[i]):
                return i
    return None


def target(tags, kind: str):
    """Index of the tag that mutate(stream, tags, kind) touches; None when the stream has no tag the mutation applies to."""
    last = len(tags) - 1
    if kind in ("offset-past", "offset-at-start"):
        return _pick(tags, lambda t: t[2] == COPY and t[1] + 1 < _OFFSET_LIMIT[t[3]] and (kind == "offset-past" or t[5] != t[1]))
    if kind == "offset-zero":
        return _pick(tags, lambda t: t[2] == COPY)
    if kind in ("offset-ffffffff", "offset-80000000"):
        return _pick(tags, lambda t: t[2] == COPY and t[3] == 4)
    if kind == "last-length+1":
        return last if tags and not (tags[last][2] == COPY and tags[last][4] == 64) else None
    if kind in ("declared+1", "extra-tag"):
        return last if tags else None
    if kind == "declared-1":
        return last if tags else None
    if kind == "cut-trailer":
        return _pick(tags, lambda t: _TRAILER[t[2], t[3]] >= 2)
    if kind == "cut-body":
        return _pick(tags, lambda t: t[2] == LIT and t[4] >= 2)
    if kind == "cut-after-tag":
        return _pick(tags, lambda t: True)
    if kind.startswith("literal-"):
        return _pick(tags, lambda t: t[1] > 0)                # before a tag that is not the first: mid-stream
    raise ValueError(kind)


def mutate(stream: bytes, tags, kind: str):
    """One grammar-aware near-miss of a stream from build(); None when target() is None.  Except for "offset-at-start" (offset = the bytes
    produced so far: the largest legal one) every kind leaves a stream that must not decode."""
    i = target(tags, kind)
    if i is None:
        return None
    ip, op, what, form, n, off = tags[i]
    s = bytearray(stream)
    hb = preamble_bytes(stream)
    if kind.startswith("offset-"):
        new = {"offset-past": op + 1, "offset-zero": 0, "offset-ffffffff": 0xFFFFFFFF, "offset-80000000": 0x80000000, "offset-at-start": op}[kind]
        s[ip: ip + 1 + _TRAILER[what, form]] = copy_tag(n, new, form)
    elif kind == "last-length+1":
        if what == LIT:
            f = max(form, min_literal_form(n + 1))
            s[ip:] = literal_header(n + 1, f) + stream[ip + 1 + form:] + b"\x00"
        else:
            f = form if form in copy_forms(n + 1, off) else 2 if off < 65536 else 4
            s[ip:] = copy_tag(n + 1, off, f)
    elif kind in ("declared+1", "declared-1"):
        total = op + n
        s[:hb] = varint(total + (1 if kind == "declared+1" else -1))
    elif kind == "cut-trailer":
        del s[ip + 2:]
    elif kind == "cut-body":
        del s[ip + 1 + form + n // 2:]
    elif kind == "cut-after-tag":
        del s[ip + 1:]
    elif kind == "extra-tag":
        s += b"\x00a"
    else:
        s[ip:ip] = bytes([0xFC]) + int(kind[8:], 16).to_bytes(4, "little")
    return bytes(s)


# ---- framed streams ------------------------------------------------------------------------------------------------------------------------
def framed(chunks, bad_crc=()) -> bytes:
    """A Snappy framed stream: the stream identifier, then one chunk per (stream, raw) pair -- compressed with `stream` as its body, or
    (stream None) uncompressed.  Chunks whose index is in bad_crc get a CRC that is off by one bit."""
    out = bytearray(FM.STREAM_ID)
    for k, (stream, raw) in enumerate(chunks):
        assert len(raw) <= B
        crc = O.crc32c(raw, masked=True) ^ (1 if k in bad_crc else 0)
        out += FM.chunk(1 if stream is None else 0, crc.to_bytes(4, "little") + (raw if stream is None else stream))
    return bytes(out)


# ---- the corpus the device tests decode (tests/test_stream_grammar.py asserts what it covers) ---------------------------------------------------
class Case:
    """One stream of the corpus: as built (mutation None: it decodes to raw) or a near-miss of it (what it gives is the oracle's to say)."""
    __slots__ = ("profile", "total", "stream", "raw", "tags", "mutation", "built")

    def __init__(self, profile, total, stream, raw, tags, mutation=None, built=None):
        self.profile, self.total, self.stream, self.raw, self.tags, self.mutation = profile, total, stream, raw, tags, mutation
        self.built = stream if built is None else built


def mutated(case: Case, k: int) -> Case:
    """The k-th kind of near-miss that applies to the stream (every stream with a tag has one)."""
    for j in range(len(MUTATIONS)):
        kind = MUTATIONS[(k + j) % len(MUTATIONS)]
        m = mutate(case.stream, case.tags, kind)
        if m is not None:
            return Case(case.profile, case.total, m, case.raw, case.tags, kind, case.stream)
    return case


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def batch_corpus(n: int = 1500, seed: int = 0, lo: int = 0, small: int = 512, big: int = 12288, full: int = 14):
    """n streams, every profile in turn: a third of 0..small output bytes, `full` of 65535 and 65536, the rest small+1..big (several super-windows
    and stages of the batch decoders each); every third one a near-miss."""
    def make():
        rnd = random.Random(f"corpus/{n}/{seed}/{lo}/{small}/{big}")
        out = []
        for i in range(n):
            profile = PROFILES[i % len(PROFILES)]
            if i >= n - full:
                total = B - (i // len(PROFILES)) % 2
            elif (i // len(PROFILES)) % 3 == 0 or big <= small:
                total = rnd.randint(lo, small)
            else:
                total = rnd.randint(small + 1, big)
            c = Case(profile, total, *build(seed * 100000 + i, total, profile))
            out.append(mutated(c, i // 3) if i % 3 == 2 else c)
        return out
    return _cached(("batch", n, seed, lo, small, big, full), make)


# Large single blocks (tests of the host API and of decompress_buffers): per profile one fragment_local stream, which the fragment decoder must
# take with no fallback, and streams it cannot take: copies from 65536 bytes back and more, tags whose output straddles a multiple of 65536.
LARGE_LOCAL = {p: 150000 + 25000 * k for k, p in enumerate(PROFILES)}          # 150000 .. 300000; two of them beyond 262144
LARGE_FOREIGN = (("far", 200000), ("far", 290000), ("uniform", 280000), ("two-slot", 270000))

# The tag index's decision for each large fragment_local stream at the kernels' sizes and pass budget: 1 = the look-back pass.  A stream of
# >= 85 % of its output goes there without a scan (snp_tag_index_look_back_only); the two that get a scan finish it on candidates alone
# (tests/test_stream_grammar.py runs tests/tag_index_model.py on each; the device test asserts the same of the kernels).
LARGE_LOOK_BACK = {"uniform": 1, "copy4": 0, "fat-literals": 1, "two-slot": 1, "pattern": 0, "dense": 1, "far": 1}


def large_local(profile: str, bounded: bool = False) -> Case:
    return _cached(("local", profile, bounded), lambda: Case(profile, LARGE_LOCAL[profile], *build(7, LARGE_LOCAL[profile], profile, fragment_local=True, bounded=bounded)))


def large_foreign(k: int) -> Case:
    profile, total = LARGE_FOREIGN[k]
    return _cached(("foreign", k), lambda: Case(profile, total, *build(7, total, profile, bounded=True)))


def large_mutated(k: int) -> Case:
    """Near-misses of large streams: a fragment_local one (the fragments fail, or the stream does not end where it declares) and a foreign one."""
    base = (large_local("copy4", True), large_foreign(0), large_local("pattern", True), large_local("two-slot", True))[k % 4]
    return _cached(("large-mutated", k), lambda: mutated(base, (1, 5, 7, 12, 0, 9, 6, 3)[k % 8]))


# Framed streams whose compressed chunks are foreign: (name, chunk recipe); a recipe entry is (profile, total), ("raw", total) for an uncompressed
# chunk, ("mutated", profile, total, k) for a near-miss as the chunk's body, ("bad-crc", profile, total) for a good body under a wrong CRC.
FRAMES = (
    ("one", (("two-slot", 4000),)),
    ("empty-then-full", (("uniform", 0), ("copy4", B))),
    ("with-uncompressed", (("uniform", 30000), ("raw", 5000), ("dense", 9000))),
    ("five", (("far", 12000), ("pattern", B), ("fat-literals", 1), ("uniform", B - 1), ("copy4", 777))),
    ("four", (("dense", 20000), ("two-slot", B), ("pattern", 300), ("fat-literals", 40000))),
    ("mutated-chunk", (("uniform", 20000), ("mutated", "copy4", 30000, 0), ("pattern", 5000))),
    ("wrong-crc", (("two-slot", 10000), ("bad-crc", "copy4", 50000))),
    ("mixed", (("raw", 1), ("uniform", 0), ("fat-literals", B), ("raw", B), ("dense", 513))),
)


def frame_corpus():
    """-> [(name, framed stream, [raw of every chunk])]; what a stream with a bad chunk gives is the oracle's to say."""
    def make():
        out = []
        for name, recipe in FRAMES:
            chunks, bad = [], []
            for k, r in enumerate(recipe):
                seed = 31 + k
                if r[0] == "raw":
                    chunks.append((None, random.Random(f"{name}/{k}").randbytes(r[1])))
                elif r[0] == "mutated":
                    c = mutated(Case(r[1], r[2], *build(seed, r[2], r[1])), r[3])
                    chunks.append((c.stream, c.raw))
                elif r[0] == "bad-crc":
                    chunks.append(build(seed, r[2], r[1])[:2])
                    bad.append(k)
                else:
                    chunks.append(build(seed, r[1], r[0])[:2])
            out.append((name, framed(chunks, bad), [raw for _s, raw in chunks]))
        return out
    return _cached("frames", make)
