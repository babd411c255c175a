"""The two device primitives everything else stands on — the exclusive scan (csrc/scan.hip) and the stable LSD radix sort on a bit range
(csrc/sort.hip) — restated in numpy with 64-bit integers, and the named inputs their tests use.  tests/test_prim_ref_cpu.py checks every
function here against a plain Python loop; tests/test_gpu_scan.py and tests/test_gpu_sort.py compare the kernels with them, exactly.

Keys are np.uint64 arrays whatever the key width of the kernel under test (a 32-bit test narrows them: the generators keep every bit at
or above `width` zero)."""
import numpy as np

U64 = np.uint64
M32 = (1 << 32) - 1
LB_VAL = (1 << 52) - 1          # scan.hip: the status words' value field; a 64-bit scan whose total reaches it is refused
TILE = 4096                     # elements of a scan tile and of a sort tile (256 threads x 16)


# ---- references ---------------------------------------------------------------------------------------------------------------------
def field(keys, b, e):
    """Bits [b, e) of every key, as uint64."""
    k = np.asarray(keys).astype(U64)
    return (k >> U64(b)) & U64((1 << (e - b)) - 1)


def sort_by_bits(keys, vals, b, e):
    """Stable sort on bits [b, e) alone: the WHOLE keys (every bit outside the range carried along) and their values in the new order."""
    w = e - b
    f = field(keys, b, e).astype(np.uint16 if w <= 16 else np.uint32 if w <= 32 else U64)      # (the narrowest type that holds the field: numpy sorts it faster)
    order = np.argsort(f, kind="stable")
    return np.asarray(keys)[order], (None if vals is None else np.asarray(vals)[order])


def excl_scan(x):
    """(exclusive prefix sums as uint64, the total as a Python int)."""
    x = np.asarray(x).astype(U64)
    if x.size == 0:
        return np.zeros(0, U64), 0
    c = np.cumsum(x, dtype=U64)
    return np.concatenate([np.zeros(1, U64), c[:-1]]), int(c[-1])


def run_starts(keys, shift):
    """Positions where keys >> shift differs from its left neighbour's (0 among them), then n."""
    k = np.asarray(keys).astype(U64) >> U64(shift)
    return np.concatenate([np.zeros(1, np.int64), np.flatnonzero(k[1:] != k[:-1]) + 1, np.array([k.size], np.int64)])


# ---- inputs of the scans ------------------------------------------------------------------------------------------------------------
SCAN_PATTERNS = ("zeros", "ones", "flags", "small", "max_first", "max_last")


def scan_input(name, n, rng):
    """uint32 inputs whose sum fits 32 bits: what every caller scans (flags, counts) and the largest sum that must be accepted."""
    x = np.zeros(n, np.uint32)
    if name == "ones":
        x[:] = 1
    elif name == "flags":
        x = rng.integers(0, 2, n, dtype=np.uint32)
    elif name == "small":
        x = rng.integers(0, (1 << 32) // n, n, dtype=np.uint64).astype(np.uint32)      # n values below 2^32 / n: the sum stays below 2^32
    elif name == "max_first":
        x[0] = M32
    elif name == "max_last":
        x[n - 1] = M32
    elif name != "zeros":
        raise ValueError(name)
    return x


def two_halves(n, i, j):
    """Zeros with 2^31 at i and at j: a sum of exactly 2^32, the smallest a 32-bit scan must refuse."""
    x = np.zeros(n, np.uint32)
    x[i] = x[j] = 1 << 31
    return x


# ---- inputs of the sorts ------------------------------------------------------------------------------------------------------------
SORT_PATTERNS = ("uniform", "const_field", "ascending", "descending", "alternating", "hot", "outside_only")


def sort_keys(name, n, b, e, width, rng):
    """n keys of `width` bits whose field [b, e) follows the pattern; every bit outside the field is random (outside_only: a counter, so
    that no two keys are equal and any reordering shows)."""
    w = e - b
    fmask = (1 << w) - 1
    i = np.arange(n, dtype=U64)
    rnd = lambda: rng.integers(0, 1 << 64, n, dtype=U64)
    if name == "uniform":
        f = rnd() & U64(fmask)
    elif name == "const_field":
        f = np.full(n, int(rng.integers(0, 1 << 62)) & fmask, U64)
    elif name in ("ascending", "descending"):
        w32 = min(w, 32)
        f = (i * U64((1 << w32) - 1) // U64(max(n - 1, 1))) << U64(w - w32)           # 0 .. the field's largest value, in order
        if name == "descending":
            f = f[::-1].copy()
    elif name == "alternating":
        x, y = (int(v) & fmask for v in rng.integers(0, 1 << 62, 2))
        if x == y:
            y = x ^ 1
        f = np.where(i & U64(1), U64(y), U64(x))
    elif name == "hot":
        f = np.where(rng.random(n) < 0.99, U64(int(rng.integers(0, 1 << 62)) & fmask), rnd() & U64(fmask))
    elif name == "outside_only":
        f = np.full(n, fmask, U64)
    else:
        raise ValueError(name)
    out = i if name == "outside_only" else rnd()
    if name == "outside_only":                                                         # the counter's bits go below b first, the rest above e
        out = (out & U64((1 << b) - 1)) | ((out >> U64(b)) << U64(e) if e < 64 else U64(0))
    wmask = (1 << width) - 1
    keep = wmask & ~(fmask << b)
    return ((out & U64(keep)) | (f << U64(b))) & U64(wmask)


# ---- inputs of the run starts -------------------------------------------------------------------------------------------------------
RUN_PATTERNS = ("single", "all_equal", "all_distinct", "sparse", "edges")
RUN_EDGES = (16, 1024, 4096, 8192)        # a thread's, a wave's, a tile's and the second tile's first element


def run_keys(name, n, shift, width, rng):
    """n keys whose `key >> shift` changes where the pattern says; the bits below shift are random (equal contexts with different payloads
    are one run).  The run index is the context; where width - shift bits cannot hold it, it wraps — neighbours still differ, which is
    all the primitive looks at."""
    new = np.zeros(n, bool)
    if name == "all_distinct":
        new[:] = True
    elif name == "sparse":
        new = rng.random(n) < 0.01
    elif name == "edges":
        new[[p for p in RUN_EDGES if p < n]] = True
    elif name == "single":
        assert n == 1
    elif name != "all_equal":
        raise ValueError(name)
    new[0] = False
    ctx = np.cumsum(new, dtype=U64) + U64(int(rng.integers(0, 2)))
    ctx &= U64((1 << (width - shift)) - 1)
    low = rng.integers(0, 1 << 64, n, dtype=U64) & U64((1 << shift) - 1)
    return (ctx << U64(shift)) | low
