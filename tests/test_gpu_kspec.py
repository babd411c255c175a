"""GPU suite of the k-mer count spectrum: k_run_spectrum through cl_kmer_spectrum_heads on constructed run starts — every bin
edge, the skew and wave shapes, the 32-bit edge, the refusals — and through the counter (cl_ctx_set_kmer_spectrum + cl_kmer_count_filter) on
the goldens, one sort and key ranges.  The judge is tests/kspec_ref.py.  head_pos is a cumulative sum of chosen run lengths: no sort is
needed and nothing beyond 4 bytes per run is allocated."""
import numpy as np
import pytest
import torch
from colord_amd import _native as N
from util import golden
import kspec_ref as K
from test_kspec_cpu import judged

pytestmark = pytest.mark.gpu


def heads_of(lengths):
    """(head_pos as the device sees it, n) of runs of the given lengths"""
    c = np.asarray(lengths, dtype=np.uint64)
    end = np.cumsum(c, dtype=np.uint64)
    n = int(end[-1]) if len(c) else 0
    assert n < 2 ** 32
    return (end - c).astype(np.uint32), n


def dev(ctx, head_pos):
    return torch.from_numpy(np.ascontiguousarray(head_pos, dtype=np.uint32).view(np.int32)).to(ctx.device)


def spectrum(ctx, lengths, max_blocks=0, acc=None):
    hp, n = heads_of(lengths)
    return ctx.kmer_spectrum_heads(dev(ctx, hp), n, max_blocks, acc).as_dict()


def check(ctx, lengths, **kw):
    got, want = spectrum(ctx, lengths, **kw), K.from_runs(lengths)
    assert K.same(got, want) is None, K.same(got, want)


EDGES = [1, 2, 8, 9, 63, 64, 65, 4094, 4095, 4096, 4097, 8191, 8192, 65535, 65536, 2 ** 20]


def test_every_bin_edge_in_one_call(ctx):
    rng = np.random.default_rng(11)
    lengths = np.array(EDGES * 3, np.uint64)
    rng.shuffle(lengths)
    check(ctx, lengths)
    want = K.from_runs(lengths)
    assert want["exact"][8] == want["exact"][9] == want["exact"][4095] == 3 and want["big"][13] == 9 and want["big"][14] == 3 and want["big"][21] == 3


@pytest.mark.parametrize("shape", ["ones_70000", "one_wave_of_100", "one_wave_of_64_lengths", "mixed_small"])
def test_skew_and_wave_shapes(ctx, shape):
    lengths = {"ones_70000": [1] * 70000,                                       # several blocks, every lane in the ballot path
               "one_wave_of_100": [100] * 64,                                   # one wave, 64 adds on one plain cell
               "one_wave_of_64_lengths": list(range(1, 65)),                    # one wave, every ballot value once and 56 different cells
               "mixed_small": list(np.random.default_rng(5).integers(1, 12, 100_003))}[shape]     # both paths in every wave, a ragged last wave
    check(ctx, lengths)


@pytest.mark.parametrize("n_heads", [1, 63, 64, 65, 255, 256, 257])
def test_tails(ctx, n_heads):
    check(ctx, [1 + (i * 7) % 11 for i in range(n_heads)])


def test_the_last_run_is_closed_by_n_near_the_32_bit_edge(ctx):
    hp = np.array([0, 5, 4100, 70000, 2 ** 31, 4_294_000_000], np.uint64)
    n = 2 ** 32 - 1
    lengths = np.diff(np.concatenate([hp, [n]]).astype(np.uint64))
    assert list(lengths) == [5, 4095, 65900, 2 ** 31 - 70000, 4_294_000_000 - 2 ** 31, 967295]
    got = ctx.kmer_spectrum_heads(dev(ctx, hp), n).as_dict()
    want = K.from_runs(lengths)
    assert K.same(got, want) is None, K.same(got, want)
    assert got["kmers"] == n and got["max_count"] == 2 ** 31 - 70000 and got["big"][31] == 2 and got["big"][20] == 1 and got["big"][17] == 1
    assert got["big_mass"][31] == 4_294_000_000 - 70000
    # a single run of the whole range
    one = ctx.kmer_spectrum_heads(dev(ctx, [0]), n).as_dict()
    assert one["big"][32] == 1 and one["big_mass"][32] == n and one["max_count"] == n and one["distinct"] == 1


def test_max_blocks_changes_nothing_and_calls_add(ctx):
    rng = np.random.default_rng(3)
    lengths = np.concatenate([np.ones(5000, np.uint64), rng.integers(1, 6000, 3000).astype(np.uint64), np.array(EDGES, np.uint64)])
    rng.shuffle(lengths)
    want = K.from_runs(lengths)
    for mb in (1, 3, 0):
        got = spectrum(ctx, lengths, max_blocks=mb)
        assert K.same(got, want) is None, (mb, K.same(got, want))
    acc = N.KSpec()
    ctx.lib.cl_kspec_clear(acc)
    spectrum(ctx, lengths[:4000], acc=acc)
    both = spectrum(ctx, lengths[4000:], acc=acc)
    assert K.same(both, want) is None, K.same(both, want)
    assert K.same(both, K.add(K.from_runs(lengths[:4000]), K.from_runs(lengths[4000:]))) is None


@pytest.mark.parametrize("how", ["equal_neighbours", "descending_pair", "last_head_at_n", "head_above_n", "more_heads_than_keys"])
def test_malformed_positions_are_refused_and_nothing_is_added(ctx, how):
    """refusals by a flag the kernel raises (or by the host's argument check): no position is used as an index, nothing is read past head_pos"""
    hp, n = heads_of([3, 1, 4, 1, 5, 9, 2, 6] * 40)
    hp = hp.copy()
    if how == "equal_neighbours":
        hp[100] = hp[99]
    elif how == "descending_pair":
        hp[200], hp[201] = hp[201], hp[200]
    elif how == "last_head_at_n":
        hp[-1] = n
    elif how == "head_above_n":
        hp[-2:] = [n + 5, n + 9]
    else:
        hp, n = np.arange(8, dtype=np.uint32), 7
    acc = N.KSpec()
    ctx.lib.cl_kspec_clear(acc)
    before = spectrum(ctx, [1, 2, 3, 5000], acc=acc)
    with pytest.raises(N.ColordHipError) as e:
        ctx.kmer_spectrum_heads(dev(ctx, hp), n, 0, acc)
    assert e.value.status == N.CL_E_INVALID
    assert K.same(acc.as_dict(), before) is None
    assert K.same(before, K.from_runs([1, 2, 3, 5000])) is None


def test_no_heads_is_ok_and_adds_nothing(ctx):
    acc = N.KSpec()
    ctx.lib.cl_kspec_clear(acc)
    got = ctx.kmer_spectrum_heads(torch.zeros(0, dtype=torch.int32, device=ctx.device), 0, 0, acc).as_dict()
    assert K.same(got, K.empty()) is None
    got = ctx.kmer_spectrum_heads(torch.zeros(0, dtype=torch.int32, device=ctx.device), 1000, 0, acc).as_dict()
    assert K.same(got, K.empty()) is None
    with pytest.raises(N.ColordHipError) as e:                                  # n >= 2^32
        ctx.kmer_spectrum_heads(dev(ctx, [0]), 2 ** 32, 0, acc)
    assert e.value.status == N.CL_E_INVALID and K.same(acc.as_dict(), K.empty()) is None


def _count(ctx, g, km):
    kset, st = ctx.count_filter(km.clone(), g.p("k"), g.p("ci"), g.p("cs"))
    keys, counts = kset.keys().cpu().numpy().view(np.uint64), kset.counts().cpu().numpy().view(np.uint32)
    kset.free()
    return st, keys, counts


@pytest.mark.parametrize("cfg", ["c1_ont_default", "c2_hifi_org", "s3m_ont_n_ratio"])
def test_through_the_counter(ctx, cfg, monkeypatch):
    g = golden(cfg)
    want = judged(cfg)
    reads = ctx.pack_readset(g.reads)
    km = ctx.kmer_scan(reads, g.p("k"), g.p("f"))
    try:
        ctx.set_kmer_spectrum(True)
        st, keys, counts = _count(ctx, g, km)
        got = ctx.kmer_spectrum()
        assert K.same(got, want) is None, K.same(got, want)
        d = K.derived(got, g.p("f"), g.p("ci"), g.p("cs"))
        assert (got["kmers"], got["distinct"], d["kept_distinct"], d["kept_kmers"]) == (st.tot_kmers, st.n_unique, st.n_unique_counted, st.total_count_filtered)
        assert np.array_equal(keys, g.kept[0]) and np.array_equal(counts, g.kept[1])          # the kept set is what it was
        if cfg == "s3m_ont_n_ratio":
            # the key-range path: about ten ranges, whose spectra add to the same
            ctx.set_kmer_spectrum(False)
            ctx.set_kmer_spectrum(True)                                         # (switching it on clears the total)
            assert K.same(ctx.kmer_spectrum(), K.empty()) is None
            monkeypatch.setenv("COLORD_HIP_COUNT_LIMIT", "60000")
            st2, keys2, counts2 = _count(ctx, g, km)
            monkeypatch.delenv("COLORD_HIP_COUNT_LIMIT")
            assert st.tot_kmers > 4 * 60000
            got2 = ctx.kmer_spectrum()
            assert K.same(got2, want) is None, K.same(got2, want)
            assert np.array_equal(keys2, g.kept[0]) and np.array_equal(counts2, g.kept[1])
        # off again: a further count adds nothing, and the total stays readable
        ctx.set_kmer_spectrum(False)
        _count(ctx, g, km)
        assert K.same(ctx.kmer_spectrum(), want) is None
    finally:
        ctx.set_kmer_spectrum(False)
        reads.free()
