"""GPU suite over the constructed read sets of tests/kmercases.py (what each case sits on is asserted there, on the CPU; the oracle they
are judged by is held against the unmodified reference's recorded results in tests/test_kmercases_cpu.py): the kernels of csrc/kmer.hip
and csrc/graph.hip against the oracle, stage by stage and case by case, bit for bit — k-mer scan (a1), count and filter (a2, also through
the key-range path of COLORD_HIP_COUNT_LIMIT), the bucket table (a3, with crafted key sets), the lists with ids, offsets and positions
(a4), the capped index and the votes (a5) in three forms: one call, batches cut by COLORD_HIP_CAND_PAIRS / COLORD_HIP_CAND_READS, and
chunks of reads (cl_index_entries_of with a reference base, cl_index_build_pairs, cl_candidates_at), and the HiFi shared k-mers.
An assertion names the stage and the read."""
import numpy as np
import pytest
import torch
import kmercases as D

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in D.CASES]
_KNOBS = ("COLORD_HIP_COUNT_LIMIT", "COLORD_HIP_CAND_PAIRS", "COLORD_HIP_CAND_READS")


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _dev64(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(ctx.device)


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)


class Stages:
    """the device's stages of one case, each made on first use; free() frees every handle"""
    def __init__(self, ctx, name):
        self.ctx, self.name, self.b = ctx, name, D.build(name)
        self.h = []
        self.reads = self._keep(ctx.pack_readset(D.readset(self.b["reads"])))
        self.has_n = np.array([(r > 3).any() for r in self.b["reads"]], bool)
        self.accept = (self.b["accept"].astype(bool) & ~self.has_n).astype(np.uint8)
        self._kset = self._lists = self._index = None

    def _keep(self, obj):
        self.h.append(obj)
        return obj

    def scan(self, reads=None):
        return self.ctx.kmer_scan(reads or self.reads, self.b["k"], self.b["f"])

    def count(self):
        """(set, statistics) of a fresh count; the caller frees the set"""
        return self.ctx.count_filter(self.scan(), self.b["k"], self.b["ci"], self.b["cs"])

    @property
    def kset(self):
        if self._kset is None:
            self._kset, self.stats = self.count()
            self._keep(self._kset)
        return self._kset

    def lists_of(self, reads):
        return self._keep(self.ctx.accepted_kmers(self.kset, reads, self.b["k"], self.b["f"]))

    @property
    def lists(self):
        if self._lists is None:
            self._lists = self.lists_of(self.reads)
        return self._lists

    @property
    def index(self):
        if self._index is None:
            self._index = self._keep(self.ctx.index_build(self.kset, self.lists, torch.from_numpy(self.accept), self.b["P"], self.b["cap"]))
        return self._index

    def pack(self, lo, hi):
        return self._keep(self.ctx.pack_readset(D.readset(self.b["reads"][lo:hi])))

    def free(self):
        for obj in reversed(self.h):
            obj.free()
        self.h = []


@pytest.fixture
def stages(ctx):
    made = []

    def make(name):
        made.append(Stages(ctx, name))
        return made[-1]
    yield make
    for s in made:
        s.free()


def check_candidates(name, refs, votes, cnt, first=0, what="candidates"):
    """rows of reads first, first + 1, ... against the oracle: count, refs, votes and the filler behind them"""
    b, o = D.build(name), D.oracle_run(name)
    refs, votes, cnt = _u32(refs), _u32(votes), _u32(cnt)
    for j in range(len(cnt)):
        i = first + j
        if i < b["P"]:
            continue                                          # a pseudo read is not coded: its row is not used
        erefs, evotes, _ = o["cands"][i]
        assert cnt[j] == len(erefs), f"{what}, read {i}: {cnt[j]} candidates, oracle {len(erefs)}"
        assert list(refs[j, :cnt[j]]) == list(erefs), f"{what}, read {i}: refs {list(refs[j])}, oracle {list(erefs)}"
        assert list(votes[j, :cnt[j]]) == list(evotes), f"{what}, read {i}: votes {list(votes[j])}, oracle {list(evotes)}"
        assert (refs[j, cnt[j]:] == 0xffffffff).all() and (votes[j, cnt[j]:] == 0).all(), f"{what}, read {i}: filler {list(refs[j])} {list(votes[j])}"


@pytest.mark.parametrize("name", NAMES)
def test_scan(stages, name):
    s, o = stages(name), D.oracle_run(name)
    got = np.sort(_u64(s.scan()))
    assert np.array_equal(got, np.sort(o["all"])), f"scan (k_kmer_scan): {len(got)} k-mers, oracle {len(o['all'])}"
    with_n = [i for i in range(len(s.b["reads"])) if s.has_n[i]]
    if with_n:                                                # the reads with N on their own: their N-free windows are counted
        sub = s._keep(s.ctx.pack_readset(D.readset([s.b["reads"][i] for i in with_n])))
        want = np.sort(np.concatenate([o["scan"][i] for i in with_n]))
        assert np.array_equal(np.sort(_u64(s.scan(sub))), want), "scan (k_kmer_scan) of the reads with N"
    for i in range(0, len(s.b["reads"]), 7):                  # and single reads: a window that leaves its read would show here
        one = s.pack(i, i + 1)
        assert np.array_equal(np.sort(_u64(s.scan(one))), np.sort(o["scan"][i])), f"scan (k_kmer_scan), read {i} alone"


def check_count(kset, st, o, what):
    assert (st.tot_kmers, st.n_unique, st.n_unique_counted, st.total_count_filtered) == o["stats"], f"{what}: statistics"
    keys, counts = _u64(kset.keys()), _u32(kset.counts())
    assert np.array_equal(keys, o["keys"]), f"{what}: kept keys (k_count_flags / k_scatter_kept): {len(keys)}, oracle {len(o['keys'])}"
    assert np.array_equal(counts, o["counts"]), f"{what}: saturated counts (k_scatter_kept)"


@pytest.mark.parametrize("name", NAMES)
def test_count_filter_and_membership(stages, name):
    s, o = stages(name), D.oracle_run(name)
    kset = s.kset
    check_count(kset, s.stats, o, "count and filter")
    keys = _u64(kset.keys())
    if len(keys):
        found = kset.check(kset.keys()).cpu().numpy()
        assert found.all(), f"table (k_table_build / table_lookup): kept keys not found {keys[found == 0][:5]}"
    others = np.setdiff1d(o["all"], o["keys"])
    others = np.concatenate([others, np.setdiff1d(o["keys"] ^ np.uint64(1), o["keys"])])
    if len(others):
        found = kset.check(_dev64(s.ctx, others)).cpu().numpy()
        assert not found.any(), f"table (table_lookup): absent keys found {others[found != 0][:5]}"


@pytest.mark.parametrize("limit", ["1", "third", "all_but_one"])
@pytest.mark.parametrize("name", D.COUNT_CASES)
def test_count_filter_by_key_ranges(stages, name, limit, monkeypatch):
    s, o = stages(name), D.oracle_run(name)
    n = len(o["all"])
    kset, st = s.count()
    s._keep(kset)
    check_count(kset, st, o, "one sort")
    monkeypatch.setenv("COLORD_HIP_COUNT_LIMIT", str({"1": 1, "third": n // 3, "all_but_one": n - 1}[limit]))
    kset2, st2 = s.count()
    s._keep(kset2)
    check_count(kset2, st2, o, f"key ranges of {limit}")
    assert torch.equal(kset.keys(), kset2.keys()) and torch.equal(kset.counts(), kset2.counts())
    if len(o["keys"]):
        assert bool(kset2.check(kset2.keys()).all()), "table over the joined ranges"


@pytest.mark.parametrize("name", D.TABLES)
def test_table_of_crafted_keys(ctx, name):
    t = D.table(name)
    keys = t["keys"]
    kset = ctx.kmer_set_from_keys(_dev64(ctx, keys), torch.ones(len(keys), dtype=torch.int32, device=ctx.device), t["k"])
    try:
        assert kset.size == len(keys) and np.array_equal(_u64(kset.keys()), np.sort(keys))
        if len(keys):
            found = kset.check(_dev64(ctx, keys)).cpu().numpy()
            assert found.all(), f"table (k_table_build / table_lookup): keys not found {keys[found == 0]}"
        found = kset.check(_dev64(ctx, t["absent"])).cpu().numpy()
        assert not found.any(), f"table (table_lookup): absent keys found {t['absent'][found != 0]}"
    finally:
        kset.free()


def test_table_ranks_of_a_wrapping_set(ctx, stages):
    """ids of the lists are the ranks the table hands out: a set of real canonical k-mers, 13 of them of the last of 16 buckets"""
    from oracle import pyoracle as O
    s = stages("table_ranks")
    keys = np.array(s.b["meta"]["keys"], np.uint64)
    kset = s._keep(ctx.kmer_set_from_keys(_dev64(ctx, keys[::-1].copy()), torch.ones(len(keys), dtype=torch.int32, device=ctx.device), s.b["k"]))
    lists = s._keep(ctx.accepted_kmers(kset, s.reads, s.b["k"], 1))
    off, kmers, ids = lists.offsets().cpu().numpy(), _u64(lists.kmers()), _u32(lists.ids())
    for i, r in enumerate(s.b["reads"]):
        want = O.accepted_kmers(r, s.b["k"], 1, keys)
        assert len(want) > 0
        assert np.array_equal(kmers[off[i]:off[i + 1]], want), f"lists (k_found_mask / table_lookup), read {i}"
        assert np.array_equal(ids[off[i]:off[i + 1]], np.searchsorted(keys, want)), f"ranks (table_lookup), read {i}"


@pytest.mark.parametrize("name", NAMES)
def test_lists(stages, name):
    s, o, m = stages(name), D.oracle_run(name), D.model(name)
    lists = s.lists
    off, kmers, ids, pos = lists.offsets().cpu().numpy(), _u64(lists.kmers()), _u32(lists.ids()), _u32(lists.pos())
    assert lists.n_reads == len(s.b["reads"]) and off[0] == 0 and off[-1] == lists.total == len(kmers)
    for i in range(len(s.b["reads"])):
        a, e = off[i], off[i + 1]
        assert e - a == len(o["lists"][i]), f"offsets (k_read_counts / k_flag_first / k_remap_offsets), read {i}: {e - a} k-mers, oracle {len(o['lists'][i])}"
        assert np.array_equal(kmers[a:e], o["lists"][i]), f"k-mers (k_emit_records / k_flag_first), read {i}"
        assert np.array_equal(ids[a:e], np.searchsorted(o["keys"], o["lists"][i])), f"ids (table_lookup), read {i}"
        assert np.array_equal(pos[a:e], m["lists"][i][1]), f"positions (k_emit_records), read {i}: {pos[a:e][:8]}, first occurrences {m['lists'][i][1][:8]}"


@pytest.mark.parametrize("name", NAMES)
def test_candidates(stages, name):
    s, o = stages(name), D.oracle_run(name)
    assert s.index.n_refs == o["n_refs"], "index (cl_index_entries_of): reference reads"
    check_candidates(name, *s.ctx.candidates(s.index, s.lists, s.b["c"]), what="one call (k_cap_flags / k_top_candidates)")


def _most_pairs(name):
    """the most vote pairs one read of the case makes (every vote of every neighbour, not cut at c)"""
    return max(sum(D.neighbours_of(name, i).values()) for i in range(len(D.build(name)["reads"])))


@pytest.mark.parametrize("form", ["pairs_1", "pairs_of_a_read", "pairs_of_a_read_less_1", "pairs_of_a_read_plus_1", "reads_1", "reads_3"])
@pytest.mark.parametrize("name", D.GRAPH_CASES)
def test_candidates_in_batches(stages, name, form, monkeypatch):
    s = stages(name)
    n = _most_pairs(name)
    assert n > 1
    knob, v = {"pairs_1": ("PAIRS", 1), "pairs_of_a_read": ("PAIRS", n), "pairs_of_a_read_less_1": ("PAIRS", n - 1), "pairs_of_a_read_plus_1": ("PAIRS", n + 1),
               "reads_1": ("READS", 1), "reads_3": ("READS", 3)}[form]
    index, lists = s.index, s.lists
    monkeypatch.setenv("COLORD_HIP_CAND_" + knob, str(v))
    check_candidates(name, *s.ctx.candidates(index, lists, s.b["c"]), what=f"batches of {v} {knob.lower()} (k_pair_fill / k_top_candidates)")


@pytest.mark.parametrize("parts", [2, 5])
@pytest.mark.parametrize("name", D.GRAPH_CASES)
def test_candidates_in_chunks(stages, name, parts):
    """the streaming and multi-GPU form: entries per chunk with the references before it as base, one index of all entries, a query per chunk"""
    s, o = stages(name), D.oracle_run(name)
    ctx, b = s.ctx, s.b
    cut = b["meta"]["chunks"][parts]
    chunks, ids, refs, base = [], [], [], 0
    for lo, hi in zip(cut, cut[1:]):
        lists = s.lists_of(s.pack(lo, hi))
        i, r, bounds, nacc = ctx.index_entries(lists, torch.from_numpy(s.accept[lo:hi].copy()), base)
        want = base + np.concatenate([[0], np.cumsum(s.accept[lo:hi])])
        assert nacc == int(s.accept[lo:hi].sum()) and np.array_equal(_u32(bounds), want), f"bounds (cl_index_entries_of), reads {lo}..{hi}"
        chunks.append((lo, lists, bounds)); ids.append(i); refs.append(r)
        base += nacc
    assert base == o["n_refs"]
    index = s._keep(ctx.index_build_pairs(s.kset, torch.cat(ids), torch.cat(refs), torch.zeros(1, dtype=torch.int32, device=ctx.device), base, b["P"], b["cap"]))
    assert index.n_refs == base
    for lo, lists, bounds in chunks:
        check_candidates(name, *ctx.candidates_at(index, lists, bounds, b["c"]), first=lo, what=f"{parts} chunks (cl_index_build_pairs / cl_candidates_at)")


def test_hifi_shared_kmers(stages):
    name = "hifi_common"
    s, o = stages(name), D.oracle_run(name)
    c = s.b["c"]
    refs, votes, cnt = s.ctx.candidates(s.index, s.lists, c)
    check_candidates(name, refs, votes, cnt)
    coff, common = s.ctx.candidates_common(s.index, s.lists, c, refs, cnt)
    coff, common = coff.cpu().numpy(), _u64(common)
    listed = 0
    for i in range(len(s.b["reads"])):
        want = o["cands"][i][2]
        for slot in range(c):
            got = common[coff[i * c + slot]:coff[i * c + slot + 1]]
            exp = want[slot] if slot < len(want) else np.zeros(0, np.uint64)
            assert np.array_equal(got, exp), f"shared k-mers (k_common), read {i} candidate {slot}: {got}, oracle {exp}"
            listed += len(exp)
    assert listed == len(common) and listed > 0
