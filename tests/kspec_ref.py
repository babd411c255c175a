"""The judge of the k-mer count spectrum, in numpy: cl_kspec as a dict from a k-mer multiset or from run lengths, the `hipkmers`
stream, and what `colord_hip info --kmer-spectrum` derives from it.  Nothing here calls the library."""
import struct
import numpy as np

EXACT = 4096
BINS = 33
WORDS = 3 + EXACT + 2 * BINS
# (field, length; 0: a scalar) in the order of cl_kspec
FIELDS = [("kmers", 0), ("distinct", 0), ("max_count", 0), ("exact", EXACT), ("big", BINS), ("big_mass", BINS)]
HEADER = ("version", "flags", "k", "f", "ci", "cs", "sets", "reserved")


def empty():
    return {k: (np.zeros(n, np.uint64) if n else 0) for k, n in FIELDS}


def from_runs(lengths):
    """the spectrum of runs of the given lengths (each >= 1): one distinct k-mer per run"""
    c = np.asarray(lengths, dtype=np.uint64)
    s = empty()
    if not len(c):
        return s
    assert int(c.min()) >= 1
    s["kmers"], s["distinct"], s["max_count"] = int(c.sum(dtype=np.uint64)), len(c), int(c.max())
    small = c[c < EXACT]
    s["exact"] = np.bincount(small.astype(np.int64), minlength=EXACT).astype(np.uint64)
    for v in c[c >= EXACT]:
        b = int(v).bit_length()
        s["big"][b] += np.uint64(1)
        s["big_mass"][b] += np.uint64(v)
    return s


def from_kmers(kmers):
    """the spectrum of a k-mer multiset"""
    _, counts = np.unique(np.asarray(kmers, dtype=np.uint64), return_counts=True)
    return from_runs(counts)


def add(a, b):
    out = {}
    for k, n in FIELDS:
        out[k] = (a[k] + b[k]) if n else (max(int(a[k]), int(b[k])) if k == "max_count" else int(a[k]) + int(b[k]))
    return out


def same(a, b):
    """None, or the first field that differs"""
    for k, n in FIELDS:
        if n:
            x, y = np.asarray(a[k], np.uint64), np.asarray(b[k], np.uint64)
            if x.shape != y.shape or not np.array_equal(x, y):
                i = int(np.nonzero(x != y)[0][0]) if x.shape == y.shape else -1
                return "%s[%d]: %s != %s" % (k, i, x[i] if i >= 0 else x.shape, y[i] if i >= 0 else y.shape)
        elif int(a[k]) != int(b[k]):
            return "%s: %d != %d" % (k, int(a[k]), int(b[k]))
    return None


def words(s):
    return np.concatenate([np.asarray(s[k], np.uint64) if n else np.array([s[k]], np.uint64) for k, n in FIELDS])


def pack_hipkmers(s, k, f, ci, cs, sets=1, flags=0, version=1, reserved=0):
    return struct.pack("<8I", version, flags, k, f, ci, cs, sets, reserved) + words(s).astype("<u8").tobytes()


def unpack_hipkmers(b):
    assert len(b) == 32 + 8 * WORDS
    h = dict(zip(HEADER, struct.unpack_from("<8I", b, 0)))
    w = np.frombuffer(b, "<u8", WORDS, 32).astype(np.uint64)
    s, at = {}, 0
    for k, n in FIELDS:
        s[k] = w[at:at + n].copy() if n else int(w[at])
        at += n or 1
    return h, s


def hist(s):
    """h[c] for the exact counts, as Python ints (h[0] = 0)"""
    return [int(x) for x in s["exact"]]


def derived(s, f, ci, cs, sets=1, flags=0):
    """what `info --kmer-spectrum` makes of a spectrum (ci <= 4096, cs < 4096)"""
    h = hist(s)
    big, mass = int(np.sum(s["big"], dtype=np.uint64)), int(np.sum(s["big_mass"], dtype=np.uint64))
    d = {}
    d["below_ci_distinct"] = sum(h[c] for c in range(1, min(ci, EXACT)))
    d["below_ci_kmers"] = sum(c * h[c] for c in range(1, min(ci, EXACT)))
    d["below_ci_distinct_share"] = d["below_ci_distinct"] / s["distinct"] if s["distinct"] else 0.0
    d["below_ci_kmers_share"] = d["below_ci_kmers"] / s["kmers"] if s["kmers"] else 0.0
    d["above_cs_distinct"] = sum(h[c] for c in range(cs + 1, EXACT)) + big
    d["saturated_kmers"] = sum((c - cs) * h[c] for c in range(cs + 1, EXACT)) + mass - cs * big
    d["kept_distinct"] = sum(h[c] for c in range(max(ci, 1), EXACT)) + big
    d["kept_kmers"] = sum(min(c, cs) * h[c] for c in range(max(ci, 1), EXACT)) + cs * big
    d["estimates"] = sets == 1 and not (flags & 1)
    if d["estimates"]:
        d["valley"] = d["peak"] = d["genome_size"] = None
        valley = next((c for c in range(1, EXACT - 1) if h[c + 1] >= h[c]), None)
        if valley is not None:
            above = sum(h[valley + 1:]) + big
            if above >= 1000:
                top = max(h[valley + 1:])
                peak = next(c for c in range(valley + 1, EXACT) if h[c] == top)
                m = sum(c * h[c] for c in range(valley + 1, EXACT)) + mass
                d.update(valley=valley, peak=peak, above_valley_distinct=above, above_valley_kmers=m, genome_size=f * m / peak)
    return d
