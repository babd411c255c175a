"""GPU suite of the k-mer MinHash sketch: k_sketch_bins / k_sketch_take through cl_kmer_sketch_runs on constructed sorted keys and
their run starts — the wave, block and take-unit edges, the cutoff bin, the ends of the hash range, the refusals — and through the counter
(cl_ctx_set_kmer_sketch + cl_kmer_count_filter) on the goldens, one sort and key ranges.  The judge is tests/sketch_ref.py; keys with chosen
hashes come from its unhash."""
import numpy as np
import pytest
import torch
from colord_amd import _native as N
from util import golden
import sketch_ref as S
from test_kspec_cpu import golden_kmers

pytestmark = pytest.mark.gpu


def layout(keys, lengths):
    """(sorted key array as the counter holds it, head_pos, n, keys ascending, their lengths) of distinct keys that occur lengths[i] times"""
    keys, c = np.asarray(keys, np.uint64), np.asarray(lengths, np.uint64)
    o = np.argsort(keys, kind="stable")
    keys, c = keys[o], c[o]
    assert len(keys) == 0 or np.all(keys[1:] > keys[:-1])
    end = np.cumsum(c, dtype=np.uint64)
    n = int(end[-1]) if len(c) else 0
    return np.repeat(keys, c.astype(np.int64)), (end - c).astype(np.uint32), n, keys, c


def dev(ctx, a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.view(np.int64 if dtype == np.uint64 else np.int32)).to(ctx.device)


def sketch(ctx, keys, lengths, size, m, max_blocks=0, acc=None):
    arr, hp, n, _, _ = layout(keys, lengths)
    acc = acc or N.Sketch(size, m)
    return ctx.kmer_sketch_runs(dev(ctx, arr, np.uint64), dev(ctx, hp, np.uint32), n, acc, max_blocks).as_dict()


def check(ctx, keys, lengths, size, m, **kw):
    got, want = sketch(ctx, keys, lengths, size, m, **kw), S.from_runs(keys, lengths, size, m)
    assert S.same(got, want) is None, S.same(got, want)
    return want


def some_keys(n, seed):
    """n distinct keys of up to 56 bits, in no order"""
    return np.random.default_rng(seed).permutation(np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F) + np.uint64(17)) & np.uint64(2 ** 56 - 1)


@pytest.mark.parametrize("n_heads", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_wave_block_and_unit_edges(ctx, n_heads):
    keys = some_keys(n_heads, n_heads)
    assert len(np.unique(keys)) == n_heads
    lengths = [1 + (i * 7) % 3 for i in range(n_heads)]                         # m - 1, m, m + 1 around m = 2, the last run among them
    want = check(ctx, keys, lengths, 50, 2)
    assert want["qualifying"] == sum(1 for c in lengths if c >= 2)
    check(ctx, keys, lengths, 10000, 2)                                         # complete: every qualifying run comes back
    check(ctx, keys, lengths, 50, 3)


def test_nothing_qualifies(ctx):
    got = sketch(ctx, some_keys(70000, 1), [1] * 70000, 100, 2)
    assert S.same(got, S.empty(100, 2)) is None and got["n"] == 0 and got["qualifying"] == 0


def test_min_count_1_takes_everything(ctx):
    keys = some_keys(5000, 2)
    lengths = [1 + (i * 5) % 4 for i in range(5000)]
    assert check(ctx, keys, lengths, 10000, 1)["qualifying"] == 5000
    check(ctx, keys, lengths, 100, 1)


@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_qualifying_around_size(ctx, extra):
    size = 300
    keys = some_keys(2000, 3)
    lengths = [2] * (size + extra) + [1] * (2000 - size - extra)
    want = check(ctx, keys, lengths, size, 2)
    assert want["qualifying"] == size + extra and len(want["hash"]) == min(size, size + extra)


@pytest.mark.parametrize("bin_", [0, 4095])
def test_every_qualifying_hash_in_one_bin(ctx, bin_):
    """the cutoff bin holds far more than size candidates: all of them are taken and sorted, the lowest size stay"""
    rng = np.random.default_rng(4 + bin_)
    low = np.unique(rng.integers(0, 2 ** 52, 2100).astype(np.uint64))[:2000]
    hashes = (np.uint64(bin_) << np.uint64(52)) | low
    keys = np.concatenate([S.unhash(hashes), S.unhash(rng.integers(2 ** 53, 2 ** 63, 3000).astype(np.uint64))])
    assert len(np.unique(keys)) == 5000
    lengths = [2 + i % 3 for i in range(2000)] + [1] * 3000
    want = check(ctx, keys, lengths, 500, 2)
    assert want["qualifying"] == 2000 and np.all(want["hash"] >> np.uint64(52) == np.uint64(bin_)) and np.array_equal(want["hash"], np.sort(hashes)[:500])


def test_the_ends_of_the_hash_range_and_neighbouring_hashes(ctx):
    rng = np.random.default_rng(6)
    hashes = np.unique(rng.integers(1, 2 ** 63, 1000).astype(np.uint64) * np.uint64(2))
    size = 200
    hashes[size] = hashes[size - 1] + np.uint64(1)                              # the size-th and the (size + 1)-th hash differ by 1
    hashes = np.concatenate([hashes, np.array([0, S.M64], np.uint64)])
    assert len(np.unique(hashes)) == len(hashes)
    keys = S.unhash(hashes)
    lengths = [2 + i % 2 for i in range(len(keys))]
    want = check(ctx, keys, lengths, size + 1, 2)                               # hash 0 first; the pair that differs by 1 is cut apart
    assert want["hash"][0] == 0 and want["hash"][-1] + np.uint64(1) == np.sort(hashes)[size + 1]
    want = check(ctx, keys, lengths, size + 2, 2)
    assert want["hash"][-1] - want["hash"][-2] == 1
    want = check(ctx, keys, lengths, 5000, 2)                                   # complete: 2^64 - 1 is the last entry
    assert want["hash"][-1] == np.uint64(S.M64) and len(want["hash"]) == len(keys)


def test_size_1_and_the_largest_size(ctx):
    keys = some_keys(9000, 7)
    lengths = [1 + (i * 3) % 9 for i in range(9000)]
    assert len(check(ctx, keys, lengths, 1, 2)["hash"]) == 1
    keys, lengths = keys[:7500], lengths[:7500]                                 # (lengths 1, 4, 7 in turn: two in three qualify)
    want = check(ctx, keys, lengths, 2 ** 20, 2)
    assert want["qualifying"] == len(want["hash"]) == 5000


def test_max_blocks_changes_nothing_and_calls_merge(ctx):
    keys = some_keys(20000, 8)
    lengths = np.array([1 + (i * 11) % 5 for i in range(20000)], np.uint64)
    want = S.from_runs(keys, lengths, 700, 2)
    for mb in (1, 3, 0):
        got = sketch(ctx, keys, lengths, 700, 2, max_blocks=mb)
        assert S.same(got, want) is None, (mb, S.same(got, want))
    # two calls over the halves of the key range give the same as one call
    o = np.argsort(keys)
    lo, hi = o[:9000], o[9000:]
    acc = N.Sketch(700, 2)
    sketch(ctx, keys[lo], lengths[lo], 700, 2, acc=acc)
    both = sketch(ctx, keys[hi], lengths[hi], 700, 2, acc=acc)
    assert S.same(both, want) is None, S.same(both, want)
    assert S.same(both, S.merge(S.from_runs(keys[lo], lengths[lo], 700, 2), S.from_runs(keys[hi], lengths[hi], 700, 2))) is None


@pytest.mark.parametrize("how", ["equal_neighbours", "descending_pair", "last_head_at_n", "head_above_n", "more_heads_than_keys", "n_2_to_32", "size_0", "size_above_2_to_20",
                                 "min_count_0"])
def test_refusals_leave_the_accumulator_as_it_was(ctx, how):
    """refusals by a flag the kernel raises or by the host's argument check: no position is used as an index, no key is loaded at one that is not
    validated, and nothing is merged"""
    keys = some_keys(320, 9)
    arr, hp, n, _, _ = layout(keys, [3, 1, 4, 1, 5, 9, 2, 6] * 40)
    hp = hp.copy()
    size, m = 40, 2
    if how == "equal_neighbours":
        hp[100] = hp[99]
    elif how == "descending_pair":
        hp[200], hp[201] = hp[201], hp[200]
    elif how == "last_head_at_n":
        hp[-1] = n
    elif how == "head_above_n":
        hp[-2:] = [n + 5, n + 9]
    elif how == "more_heads_than_keys":
        arr, hp, n = arr[:7], np.arange(8, dtype=np.uint32), 7
    elif how == "n_2_to_32":
        n = 2 ** 32
    elif how == "size_0":
        size = 0
    elif how == "size_above_2_to_20":
        size = 2 ** 20 + 1
    else:
        m = 0
    acc = N.Sketch(size, m)
    before = None
    if how not in ("size_0", "size_above_2_to_20", "min_count_0"):
        before = sketch(ctx, some_keys(100, 10), [2] * 100, size, m, acc=acc)
        assert S.same(before, S.from_runs(some_keys(100, 10), [2] * 100, size, m)) is None
    with pytest.raises(N.ColordHipError) as e:
        ctx.kmer_sketch_runs(dev(ctx, arr, np.uint64), dev(ctx, hp, np.uint32), n, acc)
    assert e.value.status == N.CL_E_INVALID
    after = acc.as_dict()
    if before is None:
        assert acc.info() == {"size": size, "min_count": m, "qualifying": 0, "n": 0}
    else:
        assert S.same(after, before) is None and after["hash"].tobytes() == before["hash"].tobytes() and after["count"].tobytes() == before["count"].tobytes()


def test_no_heads_is_ok_and_merges_nothing(ctx):
    acc = N.Sketch(10, 2)
    none8, none4 = torch.zeros(0, dtype=torch.int64, device=ctx.device), torch.zeros(0, dtype=torch.int32, device=ctx.device)
    assert S.same(ctx.kmer_sketch_runs(none8, none4, 0, acc).as_dict(), S.empty(10, 2)) is None
    assert S.same(ctx.kmer_sketch_runs(none8, none4, 1000, acc).as_dict(), S.empty(10, 2)) is None
    with pytest.raises(N.ColordHipError) as e:
        ctx.set_kmer_sketch(True, 0, 2)
    assert e.value.status == N.CL_E_INVALID
    with pytest.raises(N.ColordHipError):
        ctx.set_kmer_sketch(True, 10, 0)
    with pytest.raises(N.ColordHipError):
        ctx.set_kmer_sketch(True, 2 ** 20 + 1, 2)


def _count(ctx, g, km):
    kset, st = ctx.count_filter(km.clone(), g.p("k"), g.p("ci"), g.p("cs"))
    keys, counts = kset.keys().cpu().numpy().view(np.uint64), kset.counts().cpu().numpy().view(np.uint32)
    kset.free()
    return st, keys, counts


@pytest.mark.parametrize("cfg", ["c1_ont_default", "c2_hifi_org", "s3m_ont_n_ratio"])
def test_through_the_counter(ctx, cfg, monkeypatch):
    g = golden(cfg)
    reads = ctx.pack_readset(g.reads)
    km = ctx.kmer_scan(reads, g.p("k"), g.p("f"))
    try:
        st0, keys0, counts0 = _count(ctx, g, km)                                # the switch off
        for size, m in ((500, 2), (10000, 2), (500, 1)):
            want = S.from_kmers(golden_kmers(cfg), size, m)
            ctx.set_kmer_sketch(True, size, m)
            st, keys, counts = _count(ctx, g, km)
            got = ctx.kmer_sketch()
            assert S.same(got, want) is None, (size, m, S.same(got, want))
            assert np.array_equal(keys, g.kept[0]) and np.array_equal(counts, g.kept[1])          # the kept set is what it was
            assert np.array_equal(keys, keys0) and np.array_equal(counts, counts0)
            assert [getattr(st, f) for f, _ in N.KmerStats._fields_] == [getattr(st0, f) for f, _ in N.KmerStats._fields_]
        if cfg == "s3m_ont_n_ratio":
            # the key-range path: about ten ranges, whose sketches merge to the same
            want = S.from_kmers(golden_kmers(cfg), 500, 2)
            ctx.set_kmer_sketch(True, 500, 2)                                   # (switching it on empties the sketch)
            assert S.same(ctx.kmer_sketch(), S.empty(500, 2)) is None
            monkeypatch.setenv("COLORD_HIP_COUNT_LIMIT", "60000")
            st2, keys2, counts2 = _count(ctx, g, km)
            monkeypatch.delenv("COLORD_HIP_COUNT_LIMIT")
            assert st0.tot_kmers > 4 * 60000
            got2 = ctx.kmer_sketch()
            assert S.same(got2, want) is None, S.same(got2, want)
            assert np.array_equal(keys2, g.kept[0]) and np.array_equal(counts2, g.kept[1])
        # off again: a further count merges nothing, and the sketch stays readable
        last = ctx.kmer_sketch()
        ctx.set_kmer_sketch(False)
        _count(ctx, g, km)
        assert S.same(ctx.kmer_sketch(), last) is None
    finally:
        ctx.set_kmer_sketch(False)
        reads.free()
