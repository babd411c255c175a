"""The judge of the k-mer MinHash sketch, in numpy: the hash and its inverse, a sketch as a dict from a k-mer multiset or from
runs, the merge rule, the `hipsketch` stream, and what `colord_hip dist` makes of two sketches.  Nothing here calls the library."""
import math
import struct
import numpy as np

M64 = (1 << 64) - 1
SALT = 0x9E3779B97F4A7C15
C1, C2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
I1, I2 = pow(C1, -1, 1 << 64), pow(C2, -1, 1 << 64)
BIN_SHIFT = 52                                          # the device's 4096 cutoff bins: hash >> 52
HEADER = ("version", "flags", "k", "f", "min_count", "size", "sets", "reserved")


def hash(x):
    """cl_sketch_hash of uint64 k-mers: fmix64(x ^ SALT), vectorised (a Python int gives a Python int)"""
    if isinstance(x, int):
        return int(hash(np.array([x], np.uint64))[0])
    with np.errstate(over="ignore"):
        x = np.asarray(x, np.uint64) ^ np.uint64(SALT)
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(C1)
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(C2)
        x = x ^ (x >> np.uint64(33))
    return x


def unhash(h):
    """the k-mer of a hash: fmix64 inverted with the multiplicative inverses mod 2^64 (x ^= x >> 33 undoes itself)"""
    if isinstance(h, int):
        return int(unhash(np.array([h], np.uint64))[0])
    with np.errstate(over="ignore"):
        x = np.asarray(h, np.uint64)
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(I2)
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(I1)
        x = x ^ (x >> np.uint64(33))
    return x ^ np.uint64(SALT)


def empty(size, min_count):
    return {"size": size, "min_count": min_count, "qualifying": 0, "hash": np.zeros(0, np.uint64), "count": np.zeros(0, np.uint64)}


def from_runs(keys, lengths, size, min_count):
    """the sketch of distinct keys that occur lengths[i] times each"""
    keys, c = np.asarray(keys, np.uint64), np.asarray(lengths, np.uint64)
    assert keys.shape == c.shape and len(np.unique(keys)) == len(keys)
    q = c >= np.uint64(min_count)
    h, c = hash(keys[q]), c[q]
    o = np.argsort(h, kind="stable")[:size]
    return {"size": size, "min_count": min_count, "qualifying": int(q.sum()), "hash": h[o], "count": c[o]}


def from_kmers(kmers, size, min_count):
    """the sketch of a k-mer multiset"""
    keys, counts = np.unique(np.asarray(kmers, dtype=np.uint64), return_counts=True)
    return from_runs(keys, counts, size, min_count)


def merge(a, b):
    """union by hash, counts of equal hashes add, the lowest `size` stay; qualifying adds"""
    assert a["size"] == b["size"] and a["min_count"] == b["min_count"]
    h = np.concatenate([a["hash"], b["hash"]])
    c = np.concatenate([a["count"], b["count"]])
    u, inv = np.unique(h, return_inverse=True)
    s = np.zeros(len(u), np.uint64)
    np.add.at(s, inv, c)
    n = a["size"]
    return {"size": n, "min_count": a["min_count"], "qualifying": a["qualifying"] + b["qualifying"], "hash": u[:n], "count": s[:n]}


def same(a, b):
    """None, or the first thing that differs"""
    for k in ("size", "min_count", "qualifying"):
        if int(a[k]) != int(b[k]):
            return "%s: %d != %d" % (k, int(a[k]), int(b[k]))
    for k in ("hash", "count"):
        x, y = np.asarray(a[k], np.uint64), np.asarray(b[k], np.uint64)
        if x.shape != y.shape:
            return "%s: %d != %d entries" % (k, len(x), len(y))
        if not np.array_equal(x, y):
            i = int(np.nonzero(x != y)[0][0])
            return "%s[%d]: %d != %d" % (k, i, int(x[i]), int(y[i]))
    return None


def pack(s, k, f, sets=1, flags=0, version=1, reserved=0, n=None, qualifying=None):
    """the `hipsketch` payload (n / qualifying: a header that says something else than the entries, for the refusals)"""
    e = np.stack([np.asarray(s["hash"], np.uint64), np.asarray(s["count"], np.uint64)], axis=1).astype("<u8")
    return (struct.pack("<8I", version, flags, k, f, s["min_count"], s["size"], sets, reserved)
            + struct.pack("<2Q", s["qualifying"] if qualifying is None else qualifying, len(e) if n is None else n) + e.tobytes())


def unpack(b):
    h = dict(zip(HEADER, struct.unpack_from("<8I", b, 0)))
    q, n = struct.unpack_from("<2Q", b, 32)
    assert len(b) == 48 + 16 * n
    e = np.frombuffer(b, "<u8", 2 * n, 48).astype(np.uint64).reshape(n, 2)
    return h, {"size": h["size"], "min_count": h["min_count"], "qualifying": q, "hash": e[:, 0].copy(), "count": e[:, 1].copy()}


def dist(a, b, k):
    """what `colord_hip dist` prints of two sketches of equal k and f"""
    def top(x):
        return int(x["hash"][-1]) if len(x["hash"]) == x["size"] else M64
    t = min(top(a), top(b))
    A = set(int(x) for x in a["hash"] if int(x) <= t)
    B = set(int(x) for x in b["hash"] if int(x) <= t)
    shared, compared = len(A & B), len(A | B)
    j = shared / compared if compared else 0.0
    d = 0.0 if (compared and shared == compared) else 1.0 if not shared else -math.log(2.0 * j / (1.0 + j)) / k
    return {"shared": shared, "compared": compared, "in_a": len(A), "in_b": len(B), "jaccard": j, "containment_of_a": shared / len(A) if A else 0.0,
            "containment_of_b": shared / len(B) if B else 0.0, "distance": d}
