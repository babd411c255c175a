"""CPU suite of tests/prim_ref.py: the numpy references of the scan, the run starts and the sort on a bit range against plain Python loops
over Python integers, on every named input pattern at sizes of at most 200, and the arithmetic the overflow cases of
tests/test_gpu_scan.py rest on.  No GPU and no library: this is the yardstick's own check."""
import numpy as np
import pytest
import prim_ref as R

SIZES = (1, 2, 17, 64, 65, 200)


def loop_scan(x):
    out, acc = [], 0
    for v in x:
        out.append(acc)
        acc += int(v)
    return out, acc


def loop_sort(keys, vals, b, e):
    """Insertion of every element behind the last one whose field is not larger: stable by construction."""
    m = (1 << (e - b)) - 1
    out = []
    for k, v in zip((int(k) for k in keys), vals):
        f = (k >> b) & m
        p = len(out)
        while p > 0 and ((out[p - 1][0] >> b) & m) > f:
            p -= 1
        out.insert(p, (k, v))
    return [k for k, _ in out], [v for _, v in out]


def loop_runs(keys, shift):
    out = [0]
    for i in range(1, len(keys)):
        if int(keys[i]) >> shift != int(keys[i - 1]) >> shift:
            out.append(i)
    return out + [len(keys)]


@pytest.mark.parametrize("name", R.SCAN_PATTERNS)
def test_excl_scan_matches_loop(name):
    rng = np.random.default_rng(1)
    for n in SIZES:
        x = R.scan_input(name, n, rng)
        assert x.dtype == np.uint32 and x.size == n
        pre, total = R.excl_scan(x)
        lp, lt = loop_scan(x)
        assert pre.dtype == np.uint64 and [int(v) for v in pre] == lp and total == lt
        assert total < 1 << 32, "a pattern of the accepted kind must fit 32 bits"
        if name in ("max_first", "max_last"):
            assert total == (1 << 32) - 1
    assert R.excl_scan(np.zeros(0, np.uint32))[1] == 0 and R.excl_scan(np.zeros(0, np.uint32))[0].size == 0


def test_excl_scan_is_64_bit():
    x = np.full(200, 0xffffffff, np.uint32)
    pre, total = R.excl_scan(x)
    assert [int(v) for v in pre] == [i * 0xffffffff for i in range(200)] and total == 200 * 0xffffffff


def test_overflow_cases_arithmetic():
    m = (1 << 32) - 1
    assert R.LB_VAL == (1 << 52) - 1
    assert (1 << 20) * m < R.LB_VAL and (1 << 20) * m == (1 << 52) - (1 << 20)      # accepted, and the total the GPU test expects
    assert ((1 << 20) + 1) * m > R.LB_VAL                                           # refused
    assert ((1 << 20) + 2 * R.TILE + 1) * m - R.LB_VAL > 2 * R.TILE * m              # refused: past the limit by more than two whole tiles
    for i, j in ((0, 1), (0, 16), (0, 1024), (0, 4096)):
        x = R.two_halves(8192, i, j)
        assert x.dtype == np.uint32 and R.excl_scan(x)[1] == 1 << 32 == loop_scan(x)[1]
        assert (i // R.TILE == j // R.TILE) == (j < 4096)                           # the first three pairs share a tile, the last does not
    assert int(R.two_halves(8192, 0, 1).astype(np.uint64).sum()) & m == 0            # what a 32-bit tile sum makes of it


SORT_CASES = [(32, 0, 1), (32, 31, 32), (32, 8, 18), (32, 5, 20), (32, 8, 32), (32, 0, 32), (64, 8, 33), (64, 40, 64), (64, 63, 64), (64, 0, 64), (64, 13, 33)]


@pytest.mark.parametrize("name", R.SORT_PATTERNS)
@pytest.mark.parametrize("width,b,e", SORT_CASES)
def test_sort_by_bits_matches_loop(name, width, b, e):
    rng = np.random.default_rng(b * 64 + e)
    for n in SIZES:
        keys = R.sort_keys(name, n, b, e, width, rng)
        assert keys.dtype == np.uint64 and keys.size == n and all(int(k) < 1 << width for k in keys)
        vals = rng.permutation(n).astype(np.uint32)
        sk, sv = R.sort_by_bits(keys, vals, b, e)
        lk, lv = loop_sort(keys, vals, b, e)
        assert [int(k) for k in sk] == lk and [int(v) for v in sv] == [int(v) for v in lv]
        assert R.sort_by_bits(keys, None, b, e)[1] is None and np.array_equal(R.sort_by_bits(keys, None, b, e)[0], sk)
        f = [int(v) for v in R.field(keys, b, e)]
        assert f == [(int(k) >> b) & ((1 << (e - b)) - 1) for k in keys]
        if name in ("const_field", "outside_only"):
            assert len(set(f)) == 1 and np.array_equal(sk, keys)                    # nothing to order: the output is the input
        if name == "ascending":
            w = e - b                                                               # (the top 32 bits of a wider field run 0 .. 2^32 - 1)
            assert f == sorted(f) and (n < 2 or f[-1] >> max(0, w - 32) == (1 << min(w, 32)) - 1)
        if name == "descending":
            assert f == sorted(f, reverse=True)
        if name == "alternating" and n > 1:
            assert len(set(f)) == 2 and f[0::2] == [f[0]] * len(f[0::2])
        if name == "uniform" and n == 200 and (b > 0 or e < width):
            assert len({int(k) & ~(((1 << (e - b)) - 1) << b) for k in keys}) > 1    # live bits outside the range


def test_hot_pattern_is_hot():
    rng = np.random.default_rng(3)
    f = R.field(R.sort_keys("hot", 200, 8, 32, 32, rng), 8, 32)
    v, c = np.unique(f, return_counts=True)
    assert c.max() >= 190 and int(c.sum()) == 200


@pytest.mark.parametrize("name", R.RUN_PATTERNS)
@pytest.mark.parametrize("width,shift", [(32, 0), (32, 8), (32, 31), (64, 0), (64, 8), (64, 40)])
def test_run_starts_matches_loop(name, width, shift):
    rng = np.random.default_rng(shift)
    for n in ((1,) if name == "single" else SIZES):
        keys = R.run_keys(name, n, shift, width, rng)
        assert keys.dtype == np.uint64 and keys.size == n and all(int(k) < 1 << width for k in keys)
        got = [int(v) for v in R.run_starts(keys, shift)]
        assert got == loop_runs(keys, shift)
        if name in ("single", "all_equal"):
            assert got == [0, n]
        if name == "all_distinct":
            assert got == list(range(n + 1))
        if name == "edges":
            assert got == [0] + [p for p in R.RUN_EDGES if p < n] + [n]


def test_run_edges_at_their_size():
    """The edges pattern at the size the GPU test uses; low bits below the shift differ inside a run."""
    rng = np.random.default_rng(0)
    keys = R.run_keys("edges", 3 * R.TILE + 1, 8, 32, rng)
    assert [int(v) for v in R.run_starts(keys, 8)] == [0, 16, 1024, 4096, 8192, 3 * R.TILE + 1]
    assert len(set(int(k) for k in keys[:16])) > 1
