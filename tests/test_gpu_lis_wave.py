"""GPU suite for the wave form of the anchor chaining (k_lis_anchors_wave): tasks of at least COLORD_HIP_LIS_WAVE_MIN match
pairs are chained by a wave instead of a lane.  Both forms replay the reference's LIS, map-back scan and anchor merge, so the goldens
chained by waves only must equal the oracle, and on constructed reads every threshold must give what the lane form gives, which the
oracle judges here on the CPU."""
import numpy as np
import pytest
import torch
from oracle import pyoracle as O
import test_gpu_anchors as TA

pytestmark = pytest.mark.gpu

A_LEN, C = 16, 5
COMP = np.array([3, 2, 1, 0], np.uint8)


def _counting(ctx, monkeypatch):
    """ctx.anchor_candidates, recording the chaining counters of every call."""
    seen = []
    real = ctx.anchor_candidates

    def call(*a, **kw):
        anc = real(*a, **kw)
        seen.append(anc.lis_counts())
        return anc
    monkeypatch.setattr(ctx, "anchor_candidates", call, raising=False)
    return seen


@pytest.mark.parametrize("cfg", ["c3_clr_ratio", "s6m_ont", "s3m_ont_n_ratio", "s5m_hifi", "c7_hifi_balanced", "c2_hifi_org", "s6m_ont_k25", "s4m_ont_k23_balanced"])
def test_goldens_chained_by_waves_equal_oracle(ctx, cfg, monkeypatch):
    monkeypatch.setenv("COLORD_HIP_LIS_WAVE_MIN", "1")
    seen = _counting(ctx, monkeypatch)
    TA.test_anchor_candidates_equal_oracle(ctx, cfg)
    assert len(seen) == 1
    (wave_tasks, wave_pairs), (lane_tasks, lane_pairs) = seen[0]
    assert (lane_tasks, lane_pairs) == (0, 0), "a non-empty task went through the lane form"
    assert wave_tasks > 0 and wave_pairs >= wave_tasks


def _mmer_codes(s, a):
    n = len(s) - a + 1
    c = np.zeros(max(n, 0), np.uint64)
    for j in range(a if n > 0 else 0):
        c = (c << np.uint64(2)) | s[j:j + n].astype(np.uint64)
    return c


def _n_pairs(read, ref, a):
    ce, crs = _mmer_codes(read, a), np.sort(_mmer_codes(ref, a))
    return int((np.searchsorted(crs, ce, "right") - np.searchsorted(crs, ce, "left")).sum())


def _match_pairs(read, ref, a):
    """(read position, reference position) of every equal m-mer in the order the chaining takes them: read position ascending,
    reference position descending."""
    ce, cr = _mmer_codes(read, a), _mmer_codes(ref, a)
    order = np.argsort(cr, kind="stable")
    crs = cr[order]
    lo, hi = np.searchsorted(crs, ce, "left"), np.searchsorted(crs, ce, "right")
    e = np.repeat(np.arange(len(ce)), hi - lo)
    r = np.concatenate([order[l:h] for l, h in zip(lo, hi) if h > l] + [np.zeros(0, np.int64)]).astype(np.int64)
    k = np.lexsort((-r, e))
    return e[k], r[k]


@pytest.fixture(scope="module")
def constructed():
    """Reads, candidate lists and what the oracle makes of them (computed once, on the CPU)."""
    rng = np.random.default_rng(11)
    a = A_LEN
    genome = rng.integers(0, 4, 200_000, dtype=np.uint8)
    unit = rng.integers(0, 4, 37, dtype=np.uint8)
    genome[150_000:158_000] = np.resize(unit, 8000)                          # a tandem repeat: 37 distinct m-mers, ~200 times each
    genome[170_000:173_000] = 0                                              # and a homopolymer

    def noisy(s):
        r = rng.random(len(s))
        s = s.copy()
        sub = (r >= 0.02) & (r < 0.05)
        s[sub] = (s[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
        s = s[r >= 0.02]
        ins = np.nonzero(rng.random(len(s)) < 0.02)[0]
        return np.insert(s, ins, rng.integers(0, 4, len(ins)).astype(np.uint8))

    # noisy reads of 300 .. 70 000 bases, on either strand, that overlap each other: lists of a few to a few thousand pairs.  Then the
    # reads over the repeat and the homopolymer.  Only SHORT reads cover either of them whole: a task keeps its pairs however many they
    # are when its read has mostly distinct m-mers, as a long read has, and no kept task shall reach 100 000 pairs (checked below).
    layout = [(300, 5000), (1000, 7000), (2500, 10_000), (5000, 12_000), (12_000, 15_000), (20_000, 20_000), (30_000, 25_000), (70_000, 0),
              (21_000, 40_000), (64_000, 30_000)]
    repeat = [(9000, 148_000), (8000, 149_000), (23_000, 130_000), (15_040, 155_000)]       # whole, whole, its first and its last 3000 bases
    homo = [(5000, 169_000), (6000, 168_500)]                                              # whole; the read before ends in its first bases
    seqs = []
    for ln, st in layout + repeat + homo:
        s = noisy(genome[st:st + ln + ln // 20 + 8])[:ln]
        assert len(s) == ln
        seqs.append(COMP[s[::-1]].copy() if rng.random() < 0.5 else s)
    n_noisy = len(seqs)
    cands = []
    for i in range(n_noisy):
        cands.append([int(x) for x in rng.permutation(n_noisy) if x != i][:C])
    for i in range(len(layout)):                                             # the long reads lie over the short ones and over each other
        cands[i] = [j for j in (7, 9, 6, 5, 8, 4) if j != i][:C]
    i_rep, i_homo = len(layout), len(layout) + len(repeat)
    cands[i_rep][:3] = [i_rep + 1, i_rep + 2, i_rep + 3]; cands[i_rep + 1][:2] = [i_rep, i_rep + 3]; cands[i_rep + 2][:2] = [i_rep, 7]
    cands[i_homo][:2] = [i_homo + 1, i_rep + 3]; cands[i_homo + 1][:2] = [i_homo, i_rep + 3]; cands[i_rep + 3][:3] = [i_homo, i_rep + 1, i_rep]
    cands = [list(dict.fromkeys(cl)) for cl in cands]                        # (each candidate once)
    special = {}

    def add(name, s, cand):
        special[name] = len(seqs)
        seqs.append(np.ascontiguousarray(s, np.uint8)); cands.append(cand)

    plain = genome[180_000:192_000].copy()
    add("plain", plain, [4, 7])
    add("identical", plain.copy(), [special["plain"]])                       # one maximal run: the anchors merge into one
    add("reverse", COMP[plain[::-1]][1000:6000].copy(), [special["plain"]])  # the reference lies on the other strand
    blk = genome[192_000:198_000].copy()
    add("blocks", blk, [special["plain"]])
    add("swapped", np.concatenate([blk[3000:], blk[:3000]]), [special["blocks"]])          # the elements of the second block do not extend
    nb = noisy(genome[140_000:146_300])[:6000]
    add("blocks_noisy", nb, [special["blocks"]])
    add("swapped_noisy", noisy(np.concatenate([nb[2000:], nb[:2000]])), [special["blocks_noisy"], special["swapped"]])
    for k in (1, 2, 3):                                                      # lists of 1, 2 and 3 pairs: a shared stretch of a + k - 1 bases between mismatches
        ref = rng.integers(0, 4, 150, dtype=np.uint8)
        s = rng.integers(0, 4, 120, dtype=np.uint8)
        ln = a + k - 1
        s[30:30 + ln] = ref[50:50 + ln]
        s[29] = (ref[49] + 1) % 4; s[30 + ln] = (ref[50 + ln] + 1) % 4
        add(f"ref{k}", ref, [special["plain"]])
        add(f"pairs{k}", s, [special[f"ref{k}"]])
    n = len(seqs)
    assert sum(len(s) for s in seqs) < 600_000
    # the conditions on the inputs, from the oracle and the pair lists alone
    for k in (1, 2, 3):
        e, r = _match_pairs(seqs[special[f"pairs{k}"]], seqs[special[f"ref{k}"]], a)
        assert len(e) == k
        assert len(_match_pairs(seqs[special[f"pairs{k}"]], COMP[seqs[special[f"ref{k}"]][::-1]], a)[0]) == 0
    e, r = _match_pairs(seqs[special["identical"]], seqs[special["plain"]], a)
    assert len(e) > 128 and np.all(np.diff(r) > 0)                           # a task of more than 128 pairs, every one of which extends
    e, r = _match_pairs(seqs[special["swapped"]], seqs[special["blocks"]], a)
    assert len(e) > 128 and np.any(np.diff(r) <= 0)                          # a task with elements that do not extend
    # every task: under 100 000 pairs, or dropped for "too many matches" (more than 10 per base of a read whose m-mers repeat)
    n_veto = 0
    for i in range(n):
        distinct = len(np.unique(_mmer_codes(seqs[i], a)))
        for j in cands[i]:
            for ref in (seqs[j], COMP[seqs[j][::-1]]):
                pairs = _n_pairs(seqs[i], ref, a)
                if pairs >= 100_000:
                    assert pairs > 12 * (len(seqs[i]) + 1) and distinct < 0.8 * len(seqs[i]), f"read {i} candidate {j}: {pairs} pairs"
                    n_veto += 1
    assert n_veto >= 2
    enc = O.Encoder(a, 20, 12, 0)
    for s in seqs:
        enc.add_ref(s)
    expect = [enc.candidates(seqs[i], cands[i], None) for i in range(n)]
    assert sum(len(x) for x in expect) >= 20                                 # kept candidates
    assert sum(len(anc) for x in expect for (_, _, _, anc) in x) >= 3000     # anchors
    assert [len(anc) for (_, _, _, anc) in expect[special["identical"]]] == [1]
    assert all(len(expect[special[f"pairs{k}"]]) == 1 for k in (1, 2, 3))
    assert [x[1] for x in expect[special["reverse"]]] == [1]
    return seqs, cands, expect


def _run(ctx, reads, refs, crefs, cnt):
    anc = ctx.anchor_candidates(reads, refs, crefs, cnt, A_LEN)
    out = (anc.n_cands().cpu().numpy().copy(), anc.cands().cpu().numpy().view(np.uint32).copy(), anc.cand_offsets().cpu().numpy().copy(),
           anc.data().cpu().numpy().view(np.uint32).copy())
    counts = anc.lis_counts()
    anc.free()
    return out, counts


def test_constructed_reads_every_threshold_equals_lane_form_and_oracle(ctx, constructed, monkeypatch):
    from colord_amd.fastq import ReadSet
    seqs, cands, expect = constructed
    n = len(seqs)
    ln = np.array([len(s) for s in seqs], np.int64)
    rs = ReadSet(np.concatenate(seqs), np.concatenate([[0], np.cumsum(ln)]).astype(np.int64), None, [], [False] * n, False)
    reads = ctx.pack_readset(rs)
    refs = ctx.select_reads(reads, torch.ones(n, dtype=torch.uint8, device=ctx.device))       # every read is a reference: its id is its index
    cand = np.zeros((n, C), np.int32); cn = np.zeros(n, np.int32)
    for i, cl in enumerate(cands):
        cn[i] = len(cl); cand[i, :cn[i]] = cl
    crefs, cnt = torch.from_numpy(cand).to(ctx.device), torch.from_numpy(cn).to(ctx.device)
    monkeypatch.setenv("COLORD_HIP_LIS_WAVE_MIN", "0")
    want, (wave0, lane0) = _run(ctx, reads, refs, crefs, cnt)
    assert wave0 == (0, 0) and lane0[0] > 0 and lane0[1] > lane0[0]
    # the lane form against the oracle
    n_c, tab, off, data = want
    for i in range(n):
        assert n_c[i] == len(expect[i]), f"read {i}"
        for j, (rid, rev, tot, anchors) in enumerate(expect[i]):
            assert tuple(tab[i, j]) == (rid, rev, tot, len(anchors)), f"read {i} cand {j}"
            o = off[i * C + j]
            assert [tuple(x) for x in data[o:o + len(anchors)]] == anchors, f"read {i} cand {j}"
    # every threshold against the lane form, element for element
    for wave_min in (1, 2, 64, 65, 100000):
        monkeypatch.setenv("COLORD_HIP_LIS_WAVE_MIN", str(wave_min))
        got, (wave, lane) = _run(ctx, reads, refs, crefs, cnt)
        for w, g_, name in zip(want, got, ("n_cands", "cands", "offsets", "anchors")):
            assert np.array_equal(w, g_), f"{name} differ with COLORD_HIP_LIS_WAVE_MIN={wave_min}"
        assert (wave[0] + lane[0], wave[1] + lane[1]) == lane0, f"tasks / pairs counted with COLORD_HIP_LIS_WAVE_MIN={wave_min}"
        if wave_min == 1:
            assert wave == lane0 and lane == (0, 0)                          # every pair of every kept task went through the wave form
        if wave_min == 100000:
            assert wave == (0, 0)
        if wave_min in (64, 65):
            assert wave[0] > 0 and lane[0] > 0
    refs.free(); reads.free()
