"""The judge of the coded CIGARs in plain Python, written from the definition: symbols, contexts, the static table of a segment, the
segment bytes, and an interval encoder and decoder with the arithmetic documented in csrc/rc_dev.hpp (64-bit carry-less range coder: low 0, range
MASK at a part's start; q = range // tot, low += q * cum, range = q * freq; while range <= TOP: where low and low + range differ in their top byte the
range is cut to (low | TOP) - low, then the top byte of low goes out and both shift by 8; 8 bytes of low at the end).  Slow: small inputs only."""
import struct
import numpy as np

OPS = {1: 0, 2: 1, 7: 2, 8: 3}                               # BAM's codes of I D = X -> the op symbol
CODES = [1, 2, 7, 8]
SEG_OPS, PART_OPS = 1 << 20, 4096
BINS, ESC = 20 + 4 * 256, 255
M64 = (1 << 64) - 1
TOP, MASK = (1 << 48) - 1, 0xff << 56
LEN_MAX = (1 << 28) - 1


class Invalid(Exception):
    def __init__(self, index):
        super().__init__("word %d is no operation" % index)
        self.index = index


class Refused(Exception):
    pass


def word(op_char, n):
    return n << 4 | {"I": 1, "D": 2, "=": 7, "X": 8}[op_char]


def symbols(w):
    """(o, l, the escape or None) of a word"""
    op, n = w & 0xf, w >> 4
    return OPS[op], (n - 1 if n <= 255 else ESC), (n if n > 255 else None)


def first_invalid(words):
    for i, w in enumerate(words):
        if (int(w) & 0xf) not in OPS or int(w) >> 4 < 1:
            return i
    return None


def op_bin(row, o):
    return row * 4 + o


def len_bin(o, l):
    return 20 + o * 256 + l


def rows():
    """(first bin, symbols) of the 9 rows: the five op contexts, then the four length contexts"""
    return [(4 * r, 4) for r in range(5)] + [(20 + 256 * o, 256) for o in range(4)]


def model(counts):
    cum, tot = [0] * BINS, []
    for first, n in rows():
        t = 0
        for b in range(first, first + n):
            cum[b] = t
            t += counts[b]
        tot.append(t)
    return cum, tot


class Encoder:
    def __init__(self):
        self.low, self.range, self.out = 0, MASK, bytearray()

    def encode(self, cum, freq, tot):
        q = self.range // tot
        self.low = (self.low + q * cum) & M64
        self.range = q * freq
        while self.range <= TOP:
            if (self.low ^ ((self.low + self.range) & M64)) & MASK:
                self.range = (self.low | TOP) - self.low
            self.out.append(self.low >> 56)
            self.low = (self.low << 8) & M64
            self.range = (self.range << 8) & M64

    def end(self):
        self.out += struct.pack(">Q", self.low)
        return bytes(self.out)


class Decoder:
    def __init__(self, data):
        self.data, self.pos, self.over = data, 0, 0
        self.buffer = 0
        for _ in range(8):
            self.buffer = (self.buffer << 8) | self.byte()
        self.low, self.range = 0, MASK

    def byte(self):
        if self.pos < len(self.data):
            self.pos += 1
            return self.data[self.pos - 1]
        self.over += 1
        return 0

    def target(self, tot):
        self.range //= tot
        return self.buffer // self.range

    def update(self, cum, freq):
        r = cum * self.range
        self.buffer -= r
        self.low = (self.low + r) & M64
        self.range *= freq
        while self.range <= TOP:
            if (self.low ^ ((self.low + self.range) & M64)) & MASK:
                self.range = (self.low | TOP) - self.low
            self.buffer = ((self.buffer << 8) & M64) | self.byte()
            self.low = (self.low << 8) & M64
            self.range = (self.range << 8) & M64


def leb128(x):
    out = bytearray()
    while True:
        out.append((x & 0x7f) | (0x80 if x > 0x7f else 0))
        x >>= 7
        if not x:
            return bytes(out)


def segment_pieces(words, part_ops):
    """(counts, escapes, the parts' bytes) of one segment's words"""
    counts, escapes = [0] * BINS, []
    syms = []
    for i, w in enumerate(words):
        o, l, e = symbols(int(w))
        row = symbols(int(words[i - 1]))[0] if i % part_ops else 4
        counts[op_bin(row, o)] += 1
        counts[len_bin(o, l)] += 1
        if e is not None:
            escapes.append(e)
        syms.append((row, o, l))
    cum, tot = model(counts)
    parts = []
    for p0 in range(0, len(words), part_ops):
        e = Encoder()
        for row, o, l in syms[p0:p0 + part_ops]:
            e.encode(cum[op_bin(row, o)], counts[op_bin(row, o)], tot[row])
            e.encode(cum[len_bin(o, l)], counts[len_bin(o, l)], tot[5 + o])
        parts.append(e.end())
    return counts, escapes, parts


def segment_bytes(n_ops, part_ops, counts, escapes, parts, sizes=None, n_escapes=None, table=None):
    """the bytes of a segment from its pieces; the keyword arguments replace one field (the corrupted segments of the tests)"""
    table = b"".join(leb128(c) for c in counts) if table is None else table
    sizes = [len(p) for p in parts] if sizes is None else sizes
    head = struct.pack("<4I", n_ops, part_ops, len(escapes) if n_escapes is None else n_escapes, len(table))
    return head + struct.pack("<%dI" % len(sizes), *sizes) + table + struct.pack("<%dI" % len(escapes), *escapes) + b"".join(parts)


def pack(words, part_ops=0, seg_ops=0):
    """the segments of the words, one behind the other; Invalid names the first word that is no operation"""
    part_ops, seg_ops = part_ops or PART_OPS, seg_ops or SEG_OPS
    bad = first_invalid(words)
    if bad is not None:
        raise Invalid(bad)
    out = b""
    for s0 in range(0, len(words), seg_ops):
        seg = words[s0:s0 + seg_ops]
        out += segment_bytes(len(seg), part_ops, *segment_pieces(seg, part_ops))
    return out


def unpack(data):
    """the words of the segments in data; Refused says why"""
    words, at = [], 0
    while at < len(data):
        if len(data) - at < 16:
            raise Refused("sizes")
        n_ops, part_ops, n_esc, table_bytes = struct.unpack_from("<4I", data, at)
        if not 1 <= n_ops <= SEG_OPS or not part_ops or n_esc > n_ops:
            raise Refused("header")
        n_parts = -(-n_ops // part_ops)
        sizes_at = at + 16
        table_at = sizes_at + 4 * n_parts
        esc_at = table_at + table_bytes
        parts_at = esc_at + 4 * n_esc
        if parts_at > len(data):
            raise Refused("sizes")
        sizes = struct.unpack_from("<%dI" % n_parts, data, sizes_at)
        if parts_at + sum(sizes) > len(data):
            raise Refused("sizes")
        counts, t = [], table_at
        for _ in range(BINS):
            x, shift = 0, 0
            while True:
                if t >= esc_at or shift > 21:
                    raise Refused("table")
                c = data[t]
                t += 1
                x |= (c & 0x7f) << shift
                shift += 7
                if not c & 0x80:
                    break
            counts.append(x)
        if t != esc_at:
            raise Refused("table")
        cum, tot = model(counts)
        if sum(tot[:5]) != n_ops or tot[4] != n_parts or any(sum(counts[op_bin(r, o)] for r in range(5)) != tot[5 + o] for o in range(4)):
            raise Refused("table sum")
        if sum(counts[len_bin(o, ESC)] for o in range(4)) != n_esc:
            raise Refused("escapes")
        escapes = list(struct.unpack_from("<%dI" % n_esc, data, esc_at))
        used, p_at = 0, parts_at
        for p in range(n_parts):
            if sizes[p] < 8:
                raise Refused("part end")
            d = Decoder(data[p_at:p_at + sizes[p]])
            row = 4
            for _ in range(min(part_ops, n_ops - p * part_ops)):
                got = []
                for r in (row, None):
                    r = 5 + got[0] if r is None else r
                    if not tot[r]:
                        raise Refused("tot 0")
                    target = d.target(tot[r])
                    if target >= tot[r]:
                        raise Refused("symbol")
                    first, n = rows()[r]
                    k = first
                    while cum[k] + counts[k] <= target:
                        k += 1
                    d.update(cum[k], counts[k])
                    got.append(k - first)
                n = got[1] + 1
                if got[1] == ESC:
                    if used == n_esc:
                        raise Refused("escapes")
                    n = escapes[used]
                    used += 1
                    if n < 256 or n > LEN_MAX:
                        raise Refused("escape value")
                words.append(n << 4 | CODES[got[0]])
                row = got[0]
            if d.over or d.pos != sizes[p]:
                raise Refused("part end")
            p_at += sizes[p]
        if used != n_esc:
            raise Refused("escapes")
        at = p_at
    return np.array(words, np.uint32)


def split_segments(data):
    """[(n_ops, the segment's bytes)] by the headers alone (of bytes that unpack() accepts)"""
    out, at = [], 0
    while at < len(data):
        n_ops, part_ops, n_esc, table_bytes = struct.unpack_from("<4I", data, at)
        n_parts = -(-n_ops // part_ops)
        used = 16 + 4 * n_parts + table_bytes + 4 * n_esc + sum(struct.unpack_from("<%dI" % n_parts, data, at + 16))
        out.append((n_ops, data[at:at + used]))
        at += used
    return out


HEAD2 = 40


def pack_hipcigars2(rec_ops, segments, n_ops, n_segments):
    """the `hipcigars` stream, version 2: u32 2, u32 4, u64 records, u64 operations, u64 segments, u64 segment bytes, the counts, the segments"""
    rec_ops = np.asarray(rec_ops, "<u4")
    return struct.pack("<2I4Q", 2, 4, len(rec_ops), n_ops, n_segments, len(segments)) + rec_ops.tobytes() + segments
