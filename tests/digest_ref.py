"""The content digest restated in numpy from its definition — the yardstick of tests/test_digest_cpu.py and
tests/test_gpu_digest.py.  All arithmetic is unsigned 64-bit and wraps:

    mix(x):  x ^= x >> 30;  x *= 0xbf58476d1ce4e5b9;  x ^= x >> 27;  x *= 0x94d049bb133111eb;  x ^= x >> 31
    W(w_0 .. w_{m-1}) = sum_i mix(w_i + K (i + 1))        K = 0x9e3779b97f4a7c15
    h    = mix(W ^ mix(n + K kind))                        kind = 1 dna, 2 qual, 3 header
    sum += mix(h + K (g + 1))                              g = index of the read in the whole input

A digest is the triple (reads, symbols, sum); digests of disjoint sets of reads add field by field."""
import numpy as np

M64 = (1 << 64) - 1
K = 0x9e3779b97f4a7c15
DNA, QUAL, HEADER = 1, 2, 3
# default -T thresholds / -D values of the quality modes (usage text of `colord_hip`), by mode name
QUAL_MODES = ["org", "5-avg", "4-avg", "2-avg", "5-fix", "4-fix", "2-fix", "avg", "none"]
DEFAULT_T = {"5-avg": [7, 14, 26, 93], "4-avg": [7, 14, 26], "2-avg": [7], "5-fix": [7, 14, 26, 93], "4-fix": [7, 14, 26], "2-fix": [7]}
DEFAULT_D = {"5-fix": [3, 10, 18, 35, 93], "4-fix": [3, 10, 18, 35], "2-fix": [1, 13]}


def mix(x):
    """mix of a numpy uint64 array (or scalar)."""
    x = np.asarray(x, np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30); x *= np.uint64(0xbf58476d1ce4e5b9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94d049bb133111eb)
        x ^= x >> np.uint64(31)
    return x


def _mix1(x):
    return int(mix(np.uint64(x & M64)))


def read_term(words, n, kind, g):
    """The term of `sum` of one read: words = its uint64 words, n = its symbols."""
    words = np.asarray(words, np.uint64)
    with np.errstate(over="ignore"):
        idx = (np.arange(len(words), dtype=np.uint64) + np.uint64(1)) * np.uint64(K)
        W = int(np.sum(mix(words + idx), dtype=np.uint64)) if len(words) else 0
    h = _mix1(W ^ _mix1(n + K * kind))
    return _mix1(h + K * (g + 1))


def dna_words(codes):
    """codes: base codes 0..4 of one read -> its words (P_0, N_0, P_1, N_1, ...)."""
    codes = np.asarray(codes, np.uint8)
    n = len(codes)
    nb = (n + 31) // 32
    pad = np.zeros(nb * 32, np.uint64); pad[:n] = codes
    isn = (pad == 4)
    j = np.arange(32, dtype=np.uint64)
    two = np.where(isn, np.uint64(0), pad).reshape(nb, 32) << (np.uint64(62) - np.uint64(2) * j)
    nn = isn.reshape(nb, 32).astype(np.uint64) << (np.uint64(31) - j)
    out = np.zeros(2 * nb, np.uint64)
    out[0::2] = np.bitwise_or.reduce(two, axis=1) if nb else 0
    out[1::2] = np.bitwise_or.reduce(nn, axis=1) if nb else 0
    return out


def byte_words(b):
    """bytes of one read -> words, eight to a word little-endian, the last zero-padded."""
    b = np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else b.astype(np.uint8)
    m = (len(b) + 7) // 8
    pad = np.zeros(m * 8, np.uint8); pad[:len(b)] = b
    return pad.view("<u8").astype(np.uint64)


def add(a, b):
    return (a[0] + b[0]) & M64, (a[1] + b[1]) & M64, (a[2] + b[2]) & M64


def digest_bases(reads, first_read=0):
    """reads: list of code arrays (0..4).  -> (reads, symbols, sum)"""
    s = 0
    for i, r in enumerate(reads):
        s = (s + read_term(dna_words(r), len(r), DNA, first_read + i)) & M64
    return len(reads), sum(len(r) for r in reads), s


def digest_bytes(kind, seqs, first_read=0):
    s = 0
    for i, b in enumerate(seqs):
        s = (s + read_term(byte_words(b), len(b), kind, first_read + i)) & M64
    return len(seqs), sum(len(b) for b in seqs), s


def map_fwd(mode, thresholds=None):
    """The per-base symbol of every Phred value 0..95 under a quality mode (name): org = the value, bins: thresholds ascending,
    value v lies in bin b when T[b-1] <= v < T[b]."""
    if mode == "org":
        return np.arange(96, dtype=np.uint8)
    t = DEFAULT_T[mode] if thresholds is None else list(thresholds)
    return np.searchsorted(np.asarray(t), np.arange(96), side="right").astype(np.uint8)


def qual_symbols_fixed(mode, phred, thresholds=None):
    """org and *-fix: one symbol per base.  phred: values q - 33 of one read."""
    return map_fwd(mode, thresholds)[np.asarray(phred, np.int64)]


def digest_quals_fixed(mode, reads_phred, first_read=0, thresholds=None):
    return digest_bytes(QUAL, [qual_symbols_fixed(mode, p, thresholds) for p in reads_phred], first_read)


def parse_fastq(path):
    """-> [(id bytes, code array, phred array, plus_repeats_id)] of a four-line FASTQ."""
    code = np.full(256, 4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        code[c] = i
    out = []
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    for i in range(0, len(lines) - 3, 4):
        hid, seq, plus, q = lines[i][1:], lines[i + 1], lines[i + 2][1:], lines[i + 3]
        out.append((hid, code[np.frombuffer(seq, np.uint8)], np.frombuffer(q, np.uint8).astype(np.int64) - 33, len(plus) > 0 and plus == hid))
    return out


def parse_fasta(path):
    code = np.full(256, 4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        code[c] = i
    out = []
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    for i in range(0, len(lines) - 1, 2):
        out.append((lines[i][1:], code[np.frombuffer(lines[i + 1], np.uint8)], None, False))
    return out


def header_bytes(hid, plus):
    return bytes(hid) + bytes([1 if plus else 0])


def pack_hipdigest(dna, qual, header):
    """The `hipdigest` part: u32 version = 1, u32 flags (bit 0 dna, 1 qual, 2 header), the three triples; None = absent (zeroes, flag off)."""
    import struct
    flags = (1 if dna else 0) | (2 if qual else 0) | (4 if header else 0)
    z = (0, 0, 0)
    return struct.pack("<II9Q", 1, flags, *(dna or z), *(qual or z), *(header or z))


def unpack_hipdigest(b):
    import struct
    v = struct.unpack("<II9Q", b)
    return dict(version=v[0], flags=v[1], dna=tuple(v[2:5]), qual=tuple(v[5:8]), header=tuple(v[8:11]))
