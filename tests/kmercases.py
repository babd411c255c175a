"""Constructed read sets that put the front half of the pipeline — k-mer walk and modulo test (a1), exact count and the cut at ci / cs
(a2), the 64-byte bucket table (a3), accepted k-mers per read (a4), the k-mer -> reads index with its cap and the candidate votes (a5),
HiFi shared k-mers — on every threshold its kernels special-case (csrc/kmer.hip, csrc/graph.hip).

Three things live here, none of which uses the code under test:
  * the filter hash and its INVERSE (hash_mm is a bijection of 64-bit words), which is what makes a k-mer with a chosen hash, or a chosen
    bucket of the membership table, constructible;
  * deterministic, seeded builders of the cases (CASES: read sets with their parameters; TABLES: crafted key sets of the table);
  * a short numpy / Python model of the stage, written from the semantics of the reference (splitter.cpp:569-602 and in_reads.h:30-74:
    canonical k-mers restarted after N; hash_filter.h:8-16: hash % f == 0; kb_sorter.h:1000-1060: counts, ci, saturation at cs;
    reads_sim_graph.cpp:128-169: first occurrences per read, reads with N or shorter than k skipped; :306-317 pseudo reads uncapped;
    :381-393 votes and the capped insert; :411-418 votes descending then id ascending; :473-486,518-522 shared k-mers in read order).
The model's only purpose is to PROVE, on the CPU, that a case sits on the edge it claims (EDGES, check_edges); it is never the expected
value of a GPU test, with one exception the oracle has no output for: the position of a k-mer's first occurrence (cl_kmer_lists_pos).

What the stage must produce is the oracle's answer (oracle/kmer_graph.c), which tests/test_kmercases_cpu.py holds against the results the
unmodified reference recorded for the cases its command line can express (tests/golden/kmercases/cases.json, make_kmercases.py)."""
from __future__ import annotations
import functools
import hashlib
import json
import os
import numpy as np

M64 = (1 << 64) - 1
_C1, _C2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
_C1I, _C2I = pow(_C1, -1, 1 << 64), pow(_C2, -1, 1 << 64)


# ---- the filter hash, its inverse, k-mer helpers ------------------------------------------------------------------------
def hash_mm(x: int) -> int:
    x ^= x >> 33; x = x * _C1 & M64
    x ^= x >> 33; x = x * _C2 & M64
    return x ^ (x >> 33)


def hash_inv(h: int) -> int:
    """x with hash_mm(x) == h: y = x ^ (x >> 33) is its own inverse (2 * 33 > 64), the multipliers are odd"""
    h ^= h >> 33; h = h * _C2I & M64
    h ^= h >> 33; h = h * _C1I & M64
    return h ^ (h >> 33)


def hash_np(x: np.ndarray) -> np.ndarray:
    x = np.array(x, np.uint64)
    s = np.uint64(33)
    with np.errstate(over="ignore"):
        x ^= x >> s; x *= np.uint64(_C1)
        x ^= x >> s; x *= np.uint64(_C2)
        x ^= x >> s
    return x


def revcomp(x: int, k: int) -> int:
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3)); x >>= 2
    return r


def canon(x: int, k: int) -> int:
    return min(x, revcomp(x, k))


def kmer_bases(x: int, k: int) -> np.ndarray:
    return np.array([(x >> (2 * (k - 1 - i))) & 3 for i in range(k)], np.uint8)


def bases_kmer(b) -> int:
    x = 0
    for c in b:
        x = (x << 2) | int(c)
    return x


def rc_bases(b: np.ndarray) -> np.ndarray:
    return (3 - np.asarray(b, np.uint8)[::-1]).astype(np.uint8)


def find_all(read: np.ndarray, pat: np.ndarray):
    n, m = len(read), len(pat)
    return [i for i in range(n - m + 1) if np.array_equal(read[i:i + m], pat)]


# ---- the table's geometry (kmer.hip: bucket_of, build_table) --------------------------------------------------------------
def n_buckets(n: int) -> int:
    nb = 16
    while nb * 4 < 2 * n:
        nb <<= 1
    return nb


def bucket_of(key: int, nb: int) -> int:
    return (hash_mm(key) >> 20) & (nb - 1)


# ---- the model ------------------------------------------------------------------------------------------------------------
def windows(read: np.ndarray, k: int):
    """(start positions, canonical k-mers) of the N-free windows of a read, in read order"""
    b = np.asarray(read, np.uint8)
    n = len(b) - k + 1
    if n <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64)
    bad = np.concatenate([[0], np.cumsum(b > 3)])
    ok = (bad[k:] - bad[:-k]) == 0
    c = np.where(b > 3, 0, b).astype(np.uint64)
    fwd, rev = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(k):
        fwd = (fwd << np.uint64(2)) | c[j:j + n]
        rev |= (np.uint64(3) - c[j:j + n]) << np.uint64(2 * j)
    pos = np.nonzero(ok)[0]
    return pos, np.minimum(fwd, rev)[pos]


@functools.lru_cache(maxsize=None)
def model(name: str) -> dict:
    """scan (per read: positions, k-mers that pass the modulo test), counts, kept keys and saturated counts, lists (per read: k-mers,
    positions of the first occurrences), index (k-mer -> reference ids kept), cands (per read: refs, votes, shared k-mers a ref)"""
    b = build(name)
    k, f, ci, cs, c, P, cap = b["k"], b["f"], b["ci"], b["cs"], b["c"], b["P"], b["cap"]
    scan = []
    for r in b["reads"]:
        pos, can = windows(r, k)
        keep = hash_np(can) % np.uint64(f) == 0
        scan.append((pos[keep], can[keep]))
    allk = np.concatenate([s[1] for s in scan] + [np.zeros(0, np.uint64)])
    keys, cnt = np.unique(allk, return_counts=True)
    kept, kcnt = keys[cnt >= ci], np.minimum(cnt[cnt >= ci], cs).astype(np.uint32)
    lists = []
    for r, (pos, can) in zip(b["reads"], scan):
        if len(r) < k or (np.asarray(r) > 3).any():
            lists.append((np.zeros(0, np.uint64), np.zeros(0, np.int64))); continue
        first = np.sort(np.unique(can, return_index=True)[1])
        m = np.isin(can[first], kept)
        lists.append((can[first][m], pos[first][m]))
    index, n_refs, cands = {}, 0, []
    for i, r in enumerate(b["reads"]):
        mine = [int(x) for x in lists[i][0]]
        acc = bool(b["accept"][i]) and not (np.asarray(r) > 3).any()
        if i < P:                                             # pseudo read: always a reference, its entries uncapped
            for km in mine:
                index.setdefault(km, []).append(n_refs)
            n_refs += 1
            cands.append(([], [], [])); continue
        my = n_refs
        n_refs += acc
        votes = {}
        for km in mine:
            lst = index.setdefault(km, [])
            for ref in lst:
                votes[ref] = votes.get(ref, 0) + 1
            if acc and len(lst) < cap:
                lst.append(my)
        top = sorted(votes.items(), key=lambda e: (-e[1], e[0]))[:c]
        common = [[km for km in mine if ref in index[km]] for ref, _ in top] if b["hifi"] else []
        cands.append(([r_ for r_, _ in top], [v for _, v in top], common))
    return dict(scan=scan, keys=keys, counts=cnt, kept=kept, kept_counts=kcnt, lists=lists, index=index, cands=cands, n_refs=n_refs)


def neighbours_of(name: str, i: int) -> dict:
    """every distinct neighbour of read i with its votes (not cut at c), from the model's finished index restricted to earlier references"""
    m, b = model(name), build(name)
    before = sum(1 for j in range(i) if j < b["P"] or (b["accept"][j] and not (np.asarray(b["reads"][j]) > 3).any()))
    votes = {}
    for km in m["lists"][i][0]:
        for ref in m["index"].get(int(km), []):
            if ref < before:
                votes[ref] = votes.get(ref, 0) + 1
    return votes


# ---- builders -------------------------------------------------------------------------------------------------------------
def _rand(rng, n):
    return rng.integers(0, 4, n, dtype=np.uint8)


def _cat(*parts):
    return np.concatenate([np.asarray(p, np.uint8) for p in parts] + [np.zeros(0, np.uint8)]).astype(np.uint8)


def _with_n(read, at):
    r = np.array(read, np.uint8)
    r[list(at)] = 4
    return r


def _b_scan(c, rng):
    k = c["k"]
    marker = _rand(rng, k)
    reads, meta = [], dict(marker=canon(bases_kmer(marker), k), marker_reads=list(range(32)))
    for p in range(32):                                       # the marker starts at base p or 32 + p: every p mod 32
        reads.append(_cat(_rand(rng, p + 32 * (p % 2)), marker, _rand(rng, 3)))
    meta["lengths"] = {}
    for ln in ((0,) if c["empty"] else ()) + (k - 1, k, k + 1, 31, 32, 33, 63, 64, 65, 95, 96, 97):
        meta["lengths"].setdefault(ln, len(reads)); reads.append(_rand(rng, ln))
    a = 20
    meta["n_at"] = {}
    # "two N exactly k apart" is taken as k bases between them, a and a + k + 1: the one valid window starts at a + 1 (with the N at a
    # and a + k no window fits between, which is the read before it)
    for at in ((0,), (79,), (31,), (32,), (31, 32), (a, a + k), (a, a + k + 1)):
        meta["n_at"][at] = len(reads); reads.append(_with_n(_rand(rng, 80), at))
    return reads, meta


def _qualifies(x):
    return x < (1 << 56) and x <= revcomp(x, 28)


def _walk_down(h, step, want, pred=lambda h: True):
    """the highest hashes h, h - step, ... that satisfy pred and whose preimage is a canonical 28-mer (below 2^56 and not above its
    reverse complement: about one in 512)"""
    out = []
    while len(out) < want:
        if pred(h):
            x = hash_inv(h)
            if _qualifies(x):
                out.append(x)
        h -= step
        assert h > (1 << 63)
    return out


def _b_mod(c, rng):
    f, k = c["f"], 28
    s = (f & -f).bit_length() - 1
    d = f >> s
    top = (M64 // f) * f
    meta = dict(multiples=_walk_down(top, f, 4), near=[], partial=[], s=s, d=d, top_is_canonical=_qualifies(hash_inv(top)))
    # the preimage of a multiple's hash +- 1 is a 28-mer only one time in 512: the highest hashes of the residues 1 and f - 1 whose
    # preimages are 28-mers stand in for them
    for res in sorted({1 % f, (f - 1) % f} - {0}):
        meta["near"] += _walk_down(top - f + res, f, 2)
    if s and d > 1:
        meta["partial"] += _walk_down((M64 >> s) << s, 1 << s, 2, lambda h: h % d != 0)
        meta["partial"] += _walk_down((M64 // d) * d, d, 2, lambda h: h % (1 << s) != 0)
    reads = []
    for x in meta["multiples"] + meta["near"] + meta["partial"]:
        kb = kmer_bases(x, k)
        reads.append(_cat(_rand(rng, 7), kb, _rand(rng, 9)))
        reads.append(_cat(_rand(rng, 37), rc_bases(kb), _rand(rng, 2)))
    return reads, meta


def _place_units(rng, n_reads, units, k, extra=None):
    """reads made of the units they hold, in a random order, with fresh random spacers of k bases in front, between and behind;
    units: [(bases, [read, ...] with repeats)]"""
    per = [[] for _ in range(n_reads)]
    for u, where in units:
        for r in where:
            per[r].append(u)
    reads = []
    for lst in per:
        order = rng.permutation(len(lst))
        parts = [_rand(rng, k)]
        for j in order:
            parts += [lst[j], _rand(rng, k)]
        reads.append(_cat(*parts))
    return reads


def _b_count(c, rng):
    k, ci, cs = c["k"], c["ci"], c["cs"]
    n_reads = 3 * cs
    meta = dict(units={}, poly=[n_reads, n_reads + 1])
    units = []
    for n in sorted({ci - 1, ci, cs - 1, cs, cs + 1, 3 * cs} - {0}):
        u = _rand(rng, k + 6)
        meta["units"][n] = u
        units.append((u, list(rng.permutation(n_reads)[:n])))
    if cs >= 2:                                               # cs + 1 occurrences in cs - 1 distinct reads: three of them in the first
        u = _rand(rng, k + 6)
        where = list(rng.permutation(n_reads)[:cs - 1])
        meta["repeated"] = (u, cs - 1)
        units.append((u, where + [where[0], where[0]]))
    reads = _place_units(rng, n_reads, units, k)
    reads += [np.zeros(2 * k, np.uint8), np.full(2 * k, 3, np.uint8)]          # poly-A and poly-T: key 0 from both orientations
    return reads, meta


def _b_count_last(c, rng):
    k = c["k"]
    top = _cat(np.full(k // 2, 3), np.zeros(k // 2))          # T^(k/2) A^(k/2): its own reverse complement, the largest canonical k-mer
    reads = [_rand(rng, 90) for _ in range(6)]
    reads.insert(3, _cat(_rand(rng, 40), top, _rand(rng, 25)))
    return reads, dict(top=bases_kmer(top))


def _b_count_one(c, rng):
    return [_rand(rng, c["k"])], {}


def _b_count_run(c, rng):
    return [np.zeros(60, np.uint8)], {}


def _b_count_k6(c, rng):
    return [_rand(rng, 200) for _ in range(30)], {}


def _b_lists(c, rng):
    k = c["k"]
    d2, d3, d65 = (_rand(rng, k) for _ in range(3))
    l1, t1, t2, t3 = (_rand(rng, k + 6) for _ in range(4))
    sp = lambda: _rand(rng, 5)
    parts = [sp(), d2, sp(), rc_bases(d2), sp(), d3, sp(), rc_bases(d3), sp(), d3, sp()]
    for j in range(65):
        parts += [d65 if j % 2 == 0 else rc_bases(d65), sp()]
    dups = _cat(*parts)
    late = _cat(_rand(rng, 2100), l1)
    long3 = _cat(_rand(rng, 90), t1, _rand(rng, 2400), t2, _rand(rng, 1700), t3, _rand(rng, 100))
    nread = _with_n(_cat(sp(), d2, sp(), d3, _rand(rng, 30)), (k + 12,))
    reads = [np.zeros(0, np.uint8), dups, _rand(rng, k - 1), late, nread, long3, _rand(rng, 100), _cat(l1, _rand(rng, 30)),
             np.zeros(0, np.uint8), _cat(t3, sp(), t2, sp(), t1), _rand(rng, 100)]
    meta = dict(dups=1, d=(d2, d3, d65), times=(2, 3, 65), late=3, long3=5, empty=[0, 8], short=2, nread=4, nohit=[6, 10], full=[1, 3, 5, 7, 9])
    if not c["empty"]:                                        # the same reads without the two of 0 bases (the form the reference takes)
        at = lambda i: i - sum(1 for e in (0, 8) if e < i)
        reads = [r for i, r in enumerate(reads) if i not in (0, 8)]
        meta = {key: [at(i) for i in v] if isinstance(v, list) else at(v) if isinstance(v, int) else v for key, v in meta.items()}
        meta["empty"] = []
    return reads, meta


def _b_cap(c, rng):
    k, cap, P = c["k"], c["cs"], c["P"]
    x = {m: _rand(rng, k + 3) for m in (cap - 1, cap, cap + 1)}
    v = _rand(rng, k + 3)
    sp = lambda: _rand(rng, k)
    allx = lambda: _cat(sp(), x[cap - 1], sp(), x[cap], sp(), x[cap + 1], sp())
    reads = [allx() for _ in range(P)]
    accept = [1] * P
    hold = []
    for h in range(cap + 1):
        parts = [sp()]
        for m in x:
            if h < m:
                parts += [x[m], sp()]
        if h == cap:
            parts += [v, sp()]
        hold.append(_cat(*parts))
    na = _cat(sp(), x[cap + 1], sp())                          # not accepted, and a read with N, between the accepted ones
    nread = _with_n(allx(), (3,))
    body = [hold[0], hold[1], na, nread] + hold[2:]
    reads += body; accept += [1, 1, 0, 1] + [1] * (cap - 1)
    reads += [_rand(rng, 100), _rand(rng, 100)]; accept += [1, 1]            # accepted, no kept k-mer: empty lists
    readers = [_cat(sp(), x[m], sp()) for m in x] + [_cat(sp(), v, sp())]
    reads += readers; accept += [0] * len(readers)
    n = len(reads)
    meta = dict(x={m: bases_kmer(u[:k]) for m, u in x.items()}, v=bases_kmer(v[:k]), readers={m: n - 4 + j for j, m in enumerate(x)}, rv=n - 1,
                holders=[P, P + 1] + list(range(P + 4, P + 4 + cap - 1)),
                chunks={2: [0, P + 3, n], 5: [0, P + 2, P + 4, n - 6, n - 4, n]})
    return reads, meta, accept


def _query(rng, k, shares):
    """a query read and the units it shares: shares = [(neighbour, units)], every unit of k bases (one vote).  The spacers of a query
    are made of A and C, those of the neighbours of G and T: a k-mer that runs from a unit into a spacer differs between the two reads
    that hold the unit at its first spacer base, so a unit gives exactly one shared k-mer"""
    sp = lambda: rng.integers(0, 2, 5, dtype=np.uint8)
    parts, give = [sp()], {}
    for nb, cnt in shares:
        for _ in range(cnt):
            u = _rand(rng, k)
            give.setdefault(nb, []).append(u)
            parts += [u, sp()]
    return _cat(*parts), give


def _neighbours(rng, k, n, gives):
    sp = lambda: rng.integers(2, 4, 5, dtype=np.uint8)
    out = []
    for j in range(n):
        parts = [sp()]
        for g in gives:
            for u in g.get(j, []):
                parts += [u, sp()]
        out.append(_cat(*parts, _rand(rng, 30)))
    return out


def _tail(rng, reads):
    """two reads without a kept k-mer and two with N: chunks of empty lists and of no reference read"""
    return reads + [_rand(rng, 100), _rand(rng, 100), _with_n(_rand(rng, 100), (50,)), _with_n(_rand(rng, 100), (0,))]


def _b_votes(c, rng):
    k = c["k"]
    q = [_query(rng, k, s) for s in ([(2, 3), (0, 2), (1, 2), (3, 2)],      # c + 1 = 4 neighbours (c = 3), a tie across the third place
                                     [(0, 1), (1, 2), (3, 1)],              # exactly c neighbours
                                     [(0, 1), (1, 1), (2, 1), (3, 1)],      # all votes 1
                                     [(3, 1), (1, 1)])]                     # fewer neighbours than c
    reads = _neighbours(rng, k, 4, [g for _, g in q]) + [r for r, _ in q]
    return _tail(rng, reads), dict(queries=[4, 5, 6, 7])


def _b_votes_wide(c, rng):
    k = c["k"]
    q70, g70 = _query(rng, k, [(j, 3 if j == 64 else 1) for j in range(70)])
    q140, g140 = _query(rng, k, [(j, 3 if j == 129 else 2 if j == 66 else 1) for j in range(140)])
    nb = _neighbours(rng, k, 140, [g70, g140])
    reads = nb[:70] + [q70] + nb[70:] + [q140]
    return _tail(rng, reads), dict(q70=70, q140=141)


def _b_hifi(c, rng):
    k = c["k"]
    w, z = _rand(rng, k + 4), _rand(rng, k + 2)
    sp = lambda: _rand(rng, k)
    reads = [_cat(sp(), w, sp()) for _ in range(3)] + [_cat(sp(), w, sp(), z, sp()), _cat(sp(), z, sp(), w, sp()), _cat(sp(), z, sp())]
    return _tail(rng, reads), dict(w=w, z=z, dropped=3, q=4, q_few=5)


def _b_table_ranks(c, rng):
    """real canonical 28-mers chosen by their bucket (of 16): 13 of bucket 15, two each of buckets 0, 1 and 2, each in a read"""
    k, keys = c["k"], []
    for bucket, want in ((15, 13), (0, 2), (1, 2), (2, 2)):
        got = 0
        while got < want:
            x = canon(int(rng.integers(0, 1 << 56)), k)
            if bucket_of(x, 16) == bucket and x not in keys:
                keys.append(x); got += 1
    reads = []
    for j, x in enumerate(keys):
        kb = kmer_bases(x, k)
        reads.append(_cat(_rand(rng, j % 7), kb if j % 2 else rc_bases(kb), _rand(rng, 5)))
    reads.append(_cat(*[kmer_bases(x, k) for x in keys[::3]]))
    return reads, dict(keys=sorted(keys))


_BUILDERS = dict(scan=_b_scan, mod=_b_mod, count=_b_count, count_last=_b_count_last, count_one=_b_count_one, count_run=_b_count_run,
                 count_k6=_b_count_k6, lists=_b_lists, cap=_b_cap, votes=_b_votes, votes_wide=_b_votes_wide, hifi=_b_hifi,
                 table_ranks=_b_table_ranks)

MOD_F = (1, 2, 3, 4, 5, 6, 7, 8, 12, 24, 40, 96, 1000, 4096, 3 << 16, 1 << 31, (1 << 32) - 1)
# The divide-free test (common.hpp: mod_is_zero) compares a quotient with lim = (2^64 - 1) / d and meets equality for ONE hash only, the
# highest multiple of an odd f.  Its preimage is a canonical 28-mer for none of the f above (one time in 512); 2933 and 3019 are the
# first odd f for which it is.
MOD_F_LIM = (2933, 3019)


def _case(name, kind, seed, k=20, f=1, ci=2, cs=80, c=5, hifi=False, P=0, record=True, empty=False):
    return dict(name=name, kind=kind, seed=seed, k=k, f=f, ci=ci, cs=cs, c=c, hifi=hifi, P=P, record=record, empty=empty)


_K15 = "k < 15: the reference's command line takes k from 15 to 28"
_EMPTY = "a read of 0 bases, which the reference's FASTQ reader refuses"


# record: True = the reference's results are in tests/golden/kmercases/cases.json; otherwise the reason the case is oracle-only
CASES = (
    [_case(f"scan_k{k}", "scan", 100 + k, k=k, ci=1, empty=k in (1, 16), record=_K15 if k < 15 else _EMPTY if k == 16 else True)
     for k in (1, 15, 16, 27, 28)]
    + [_case(f"mod_f{f}", "mod", 200 + i, k=28, f=f, ci=1) for i, f in enumerate(MOD_F + MOD_F_LIM)]
    + [_case(f"count_ci{ci}_cs{cs}", "count", 300 + ci, ci=ci, cs=cs) for ci, cs in ((1, 2), (2, 5), (4, 80))]
    + [_case("count_k28_last", "count_last", 310, k=28, ci=1),
       _case("count_one_kmer", "count_one", 311, ci=1),
       _case("count_one_run", "count_run", 312, ci=1),
       _case("count_k6", "count_k6", 313, k=6, cs=5, record=_K15),
       _case("lists_all", "lists", 400, empty=True, record=_EMPTY), _case("lists_no_empty", "lists", 400)]
    + [_case(f"cap_p{P}", "cap", 500 + P, cs=4, c=6, P=P,
             record="explicit accept flags" + (" and pseudo reads, which need a genome whose cutting yields them" if P else ""))
       for P in (0, 3, 4, 5)]
    + [_case("votes_c3", "votes", 600, c=3), _case("votes_c1", "votes", 600, c=1), _case("votes_wide", "votes_wide", 602, c=5),
       _case("hifi_common", "hifi", 700, cs=3, c=4, hifi=True),
       _case("table_ranks", "table_ranks", 800, k=28, ci=1, record="crafted table keys: the set is given, not counted")]
)
BY_NAME = {c["name"]: c for c in CASES}
GRAPH_CASES = [c["name"] for c in CASES if c["kind"] in ("cap", "votes", "votes_wide", "hifi")]
COUNT_CASES = [c["name"] for c in CASES if c["kind"].startswith("count")]


@functools.lru_cache(maxsize=None)
def build(name: str) -> dict:
    c = BY_NAME[name]
    out = _BUILDERS[c["kind"]](c, np.random.default_rng(c["seed"]))
    reads, meta = out[0], out[1]
    accept = np.asarray(out[2] if len(out) > 2 else [1] * len(reads), np.uint8)
    for r in reads:
        r.setflags(write=False)
    if "chunks" not in meta:
        meta["chunks"] = {p: [int(x) for x in np.linspace(0, len(reads), p + 1)] for p in (2, 5)}
    return dict(c, reads=reads, accept=accept, cap=c["cs"], meta=meta)     # the index cap is maxKmerCount, i.e. cs (reads_sim_graph.cpp:390)


def readset(reads):
    from colord_amd.fastq import ReadSet
    lens = [len(r) for r in reads]
    return ReadSet(_cat(*reads), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), None, [], [], False)


def fastq_bytes(name: str) -> bytes:
    """the case as the FASTQ file handed to the reference"""
    lut = np.frombuffer(b"ACGTN", np.uint8)
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, lut[r].tobytes(), b"I" * len(r)) for i, r in enumerate(build(name)["reads"]))


def input_sha(name: str) -> str:
    return hashlib.sha256(fastq_bytes(name)).hexdigest()


def ref_args(name: str):
    c = BY_NAME[name]
    # (-a: the anchor length must come with -k and not exceed it, nothing recorded here depends on it; -R all: every read without N is a
    # reference read, as in the cases, where the presets would draw them sparsely)
    return ["compress-pbhifi" if c["hifi"] else "compress-ont", "-k", str(c["k"]), "-a", str(c["k"] - 4), "-L", str(c["ci"]), "-H", str(c["cs"]),
            "-f", str(c["f"]), "-c", str(c["c"]), "-R", "all"]


@functools.lru_cache(maxsize=None)
def golden_cases() -> dict:
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmercases", "cases.json")
    return {c["name"]: c for c in json.load(open(path))["cases"]}


def sha_u(a, dtype) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, dtype).tobytes()).hexdigest()


def cands_digest(cands) -> str:
    """cands: per read (refs, shared k-mers a ref or [])"""
    h = hashlib.sha256()
    for refs, common in cands:
        h.update(np.asarray([len(refs)] + [int(r) for r in refs], "<u4").tobytes())
        for cm in common:
            h.update(np.asarray([len(cm)], "<u4").tobytes()); h.update(np.asarray(cm, "<u8").tobytes())
    return h.hexdigest()


# ---- the oracle's answer for a case -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_run(name: str) -> dict:
    from oracle import pyoracle as O
    b = build(name)
    k, f = b["k"], b["f"]
    scan = [O.kmer_scan(r, k, f) for r in b["reads"]]
    allk = np.concatenate(scan + [np.zeros(0, np.uint64)])
    keys, counts, st = O.count_filter(allk, b["ci"], b["cs"])
    lists = [O.accepted_kmers(r, k, f, keys) for r in b["reads"]]
    g = O.Graph(b["c"], b["cap"])
    cands = []
    for i, r in enumerate(b["reads"]):
        if i < b["P"]:
            g.add_pseudo(lists[i]); cands.append((np.zeros(0, np.uint32), np.zeros(0, np.uint32), [])); continue
        acc = bool(b["accept"][i]) and not (r > 3).any()
        refs, votes, common = g.next_read(lists[i], acc, b["hifi"])
        cands.append((refs, votes, common or []))
    return dict(scan=scan, all=allk, keys=keys, counts=counts, stats=(st.tot_kmers, st.n_unique, st.n_unique_counted, st.total_count_filtered),
                lists=lists, cands=cands, n_refs=int(O.lib().orc_graph_n_refs(g.h)))


# ---- crafted key sets of the membership table -----------------------------------------------------------------------------
def _keys_of_bucket(rng, nb, bucket, want, taken):
    out = []
    while len(out) < want:
        x = int(rng.integers(0, 1 << 56))
        if bucket_of(x, nb) == bucket and x not in taken and x not in out:
            out.append(x)
    return out


def _keys_avoiding(rng, nb, avoid, want, taken):
    out = []
    while len(out) < want:
        x = int(rng.integers(0, 1 << 56))
        if bucket_of(x, nb) not in avoid and x not in taken and x not in out:
            out.append(x)
    return out


TABLES = ("table_wrap", "table_4", "table_5", "table_n0", "table_n1", "table_n32", "table_n33", "table_extremes")


@functools.lru_cache(maxsize=None)
def table(name: str) -> dict:
    """keys (k = 28, below 2^56) and constructed absent keys of one table"""
    rng = np.random.default_rng(900 + TABLES.index(name))
    keys, absent = [], []
    if name == "table_wrap":                                  # 13 keys of bucket 15: nine spill into buckets 0, 1, 2 (two own keys each) and 3
        keys = _keys_of_bucket(rng, 16, 15, 13, [])
        for bk in (0, 1, 2):
            keys += _keys_of_bucket(rng, 16, bk, 2, keys)
        for bk in (15, 15, 15, 0, 1, 2, 3, 14):
            absent += _keys_of_bucket(rng, 16, bk, 1, keys + absent)
    elif name in ("table_4", "table_5"):
        n = int(name[-1])
        keys = _keys_of_bucket(rng, 16, 7, n, []) + _keys_of_bucket(rng, 16, 8, 4 if n == 5 else 1, [])
        keys += _keys_avoiding(rng, 16, (7, 8, 9), 3, keys)
        for bk in (7, 7, 8, 6):
            absent += _keys_of_bucket(rng, 16, bk, 1, keys + absent)
    elif name == "table_extremes":
        keys = [0, (1 << 56) - 1] + _keys_avoiding(rng, 16, (), 5, [0, (1 << 56) - 1])
        absent = [1, (1 << 56) - 2] + _keys_avoiding(rng, 16, (), 6, keys + [1, (1 << 56) - 2])
    else:
        n = int(name[7:])
        keys = _keys_avoiding(rng, 16, (), n, [])
        absent = _keys_avoiding(rng, 16, (), 40, keys)
    return dict(k=28, keys=np.array(keys, np.uint64), absent=np.array(absent, np.uint64))


def table_fill(name: str):
    """(buckets, keys whose home is each bucket, slots taken in each bucket after linear probing over buckets: whatever order the keys
    are placed in, a bucket ends with min(4, own + spilled in) keys)"""
    t = table(name)
    nb = n_buckets(len(t["keys"]))
    home = np.bincount([bucket_of(int(x), nb) for x in t["keys"]], minlength=nb)
    fill = np.zeros(nb, np.int64)
    carry, start = 0, int(np.argmin(home))                    # an emptiest bucket: nothing spills past it at load <= 1/2... checked below
    for step in range(2 * nb):
        bk = (start + step) % nb
        tot = carry + (home[bk] if step < nb else 0)
        add = min(4 - fill[bk], tot)
        fill[bk] += add
        carry = tot - add
    assert carry == 0 and fill.sum() == len(t["keys"])
    return nb, home, fill


# ---- the edges --------------------------------------------------------------------------------------------------------------
def _e_scan_marker_offsets():
    held = []
    for k in (1, 15, 16, 27, 28):
        n = f"scan_k{k}"
        b, m = build(n), model(n)
        seen = set()
        for i in b["meta"]["marker_reads"]:
            pos, can = m["scan"][i]
            seen |= {int(p) % 32 for p, x in zip(pos, can) if int(x) == b["meta"]["marker"]}
        assert seen == set(range(32)), n
        held.append(n)
    return held


def _e_scan_lengths():
    held = []
    for k in (1, 15, 16, 27, 28):
        n = f"scan_k{k}"
        b, m = build(n), model(n)
        lens = [len(r) for r in b["reads"]]
        assert {k - 1, k, k + 1} <= set(lens) and {0, 1, 31} <= {ln % 32 for ln in lens if ln >= k} and (0 in lens) == b["empty"], n
        for ln in (k - 1, k, k + 1):
            assert len(m["scan"][b["meta"]["lengths"][ln]][0]) == max(0, ln - k + 1)
        held.append(n)
    return held


def _e_scan_n():
    held = []
    for k in (1, 15, 16, 27, 28):
        n = f"scan_k{k}"
        b, m = build(n), model(n)
        at = b["meta"]["n_at"]
        assert set(at) >= {(0,), (79,), (31,), (32,), (31, 32)}
        for pos_n, i in at.items():
            r = b["reads"][i]
            assert len(r) == 80 and sorted(np.nonzero(r > 3)[0]) == list(pos_n)
            assert len(m["lists"][i][0]) == 0                 # a read with N has no list
            pos = m["scan"][i][0]
            exp = [p for p in range(80 - k + 1) if not any(p <= q < p + k for q in pos_n)]
            assert list(pos) == exp and len(exp) > 0, (n, pos_n)     # ... but its N-free windows are counted
        a = 20
        between = lambda pn: [p for p in m["scan"][at[pn]][0] if a < p and p + k <= pn[1]]
        assert between((a, a + k)) == [] and between((a, a + k + 1)) == [a + 1], n
        held.append(n)
    return held


def _e_mod(which):
    def check():
        held = []
        for f in MOD_F + MOD_F_LIM:
            n = f"mod_f{f}"
            b, m = build(n), model(n)
            me = b["meta"]
            scanned = {int(x) for s in m["scan"] for x in s[1]}
            if which == "multiples":
                assert len(me["multiples"]) >= 4
                for x in me["multiples"]:
                    assert canon(x, 28) == x and hash_mm(x) % f == 0 and x in scanned, n
                hs = sorted(hash_mm(x) for x in me["multiples"])
                assert hs[0] > M64 - 5000 * f * 4                 # all of them within a few thousand multiples of 2^64
            elif which == "near":
                if f <= 2 and not me["near"]:
                    continue                                      # f = 1: every residue is 0
                for x in me["near"]:
                    assert hash_mm(x) % f in (1, f - 1) and hash_mm(x) % f != 0 and x not in scanned, n
            else:
                if not (me["s"] and me["d"] > 1):
                    continue
                assert len(me["partial"]) == 4
                for j, x in enumerate(me["partial"]):
                    h = hash_mm(x)
                    assert (h % (1 << me["s"]) == 0) == (j < 2) and (h % me["d"] == 0) == (j >= 2) and x not in scanned, n
            held.append(n)
        return held
    return check


def _e_mod_lim():
    held = []
    for f in MOD_F:
        assert not build(f"mod_f{f}")["meta"]["top_is_canonical"]
    for f in MOD_F_LIM:
        n = f"mod_f{f}"
        me, m = build(n)["meta"], model(n)
        x = me["multiples"][0]
        assert f % 2 == 1 and me["top_is_canonical"] and hash_mm(x) // f == M64 // f and hash_mm(x) % f == 0 and hash_mm(x) + f > M64
        assert x in {int(y) for s in m["scan"] for y in s[1]}
        held.append(n)
    return held


def _unit_kmers(u, k):
    return [int(x) for x in windows(u, k)[1]]


def _e_count_units():
    held = []
    for n in ("count_ci1_cs2", "count_ci2_cs5", "count_ci4_cs80"):
        b, m = build(n), model(n)
        ci, cs, k = b["ci"], b["cs"], b["k"]
        cnt = dict(zip((int(x) for x in m["keys"]), (int(x) for x in m["counts"])))
        assert set(b["meta"]["units"]) == {ci - 1, ci, cs - 1, cs, cs + 1, 3 * cs} - {0}
        kept = {int(x): int(y) for x, y in zip(m["kept"], m["kept_counts"])}
        for want, u in b["meta"]["units"].items():
            for x in _unit_kmers(u, k):
                assert cnt[x] == want and (x in kept) == (want >= ci) and (want < ci or kept[x] == min(want, cs)), (n, want)
        held.append(n)
    return held


def _e_count_repeated():
    held = []
    for n in ("count_ci1_cs2", "count_ci2_cs5", "count_ci4_cs80"):
        b, m = build(n), model(n)
        u, in_reads = b["meta"]["repeated"]
        for x in _unit_kmers(u, b["k"]):
            tot = sum(int((s[1] == np.uint64(x)).sum()) for s in m["scan"])
            reads = sum(1 for s in m["scan"] if (s[1] == np.uint64(x)).any())
            assert tot == b["cs"] + 1 and reads == b["cs"] - 1 == in_reads, n
        held.append(n)
    return held


def _e_count_poly():
    held = []
    for n in ("count_ci1_cs2", "count_ci2_cs5", "count_ci4_cs80", "count_one_run"):
        b, m = build(n), model(n)
        assert int(m["keys"][0]) == 0 and int(m["kept"][0]) == 0
        if n != "count_one_run":
            a, t = b["meta"]["poly"]
            assert (b["reads"][a] == 0).all() and (b["reads"][t] == 3).all() and len(m["scan"][a][1]) == len(m["scan"][t][1]) > 0
            assert (m["scan"][a][1] == 0).all() and (m["scan"][t][1] == 0).all()
        held.append(n)
    return held


def _e_count_last_single():
    b, m = build("count_k28_last"), model("count_k28_last")
    assert int(m["keys"][-1]) == b["meta"]["top"] == int(m["kept"][-1]) and int(m["counts"][-1]) == 1
    assert all(canon(x, 28) <= b["meta"]["top"] for x in (b["meta"]["top"] + 1, (1 << 56) - 1, b["meta"]["top"] + 5))
    return ["count_k28_last"]


def _e_count_one_kmer():
    m = model("count_one_kmer")
    assert len(m["keys"]) == 1 and int(m["counts"][0]) == 1 and len(m["scan"]) == 1
    return ["count_one_kmer"]


def _e_count_one_run():
    m = model("count_one_run")
    assert len(m["keys"]) == 1 and int(m["counts"][0]) == 41
    return ["count_one_run"]


def _e_count_k6():
    b, m = build("count_k6"), model("count_k6")
    assert 2 * b["k"] <= 12 and (m["counts"] < b["ci"]).any() and (m["counts"] > b["cs"]).any() and (m["counts"] == b["cs"]).any()
    return ["count_k6"]


def _e_table(name, check):
    def run():
        nb, home, fill = table_fill(name)
        check(table(name), nb, home, fill)
        return [name]
    return run


def _t_wrap(t, nb, home, fill):
    assert nb == 16 and home[15] == 13 and list(home[:3]) == [2, 2, 2] and list(fill[[15, 0, 1, 2, 3]]) == [4, 4, 4, 4, 3]
    ab = [bucket_of(int(x), nb) for x in t["absent"]]
    assert ab.count(15) == 3 and {0, 1, 2} <= set(ab)            # home bucket full, and the next one too: the walk ends in bucket 3


def _t_4(t, nb, home, fill):
    assert nb == 16 and home[7] == 4 and fill[7] == 4 and fill[8] == 1 and bucket_of(int(t["absent"][0]), nb) == 7


def _t_5(t, nb, home, fill):
    assert nb == 16 and home[7] == 5 and home[8] == 4 and fill[7] == 4 and fill[8] == 4 and fill[9] == 1
    assert [bucket_of(int(x), nb) for x in t["absent"][:3]] == [7, 7, 8]


def _t_n(n, buckets):
    def check(t, nb, home, fill):
        assert len(t["keys"]) == n and nb == buckets
    return check


def _t_extremes(t, nb, home, fill):
    assert {0, (1 << 56) - 1} <= {int(x) for x in t["keys"]} and nb == 16


def _e_table_ranks():
    b, m = build("table_ranks"), model("table_ranks")
    keys = b["meta"]["keys"]
    home = np.bincount([bucket_of(x, 16) for x in keys], minlength=16)
    assert len(keys) == 19 and home[15] == 13 and list(home[:3]) == [2, 2, 2] and all(canon(x, 28) == x for x in keys)
    scanned = {int(x) for s in m["scan"] for x in s[1]}
    assert set(keys) <= scanned
    return ["table_ranks"]


def _both_lists(fn):
    def run():
        for n in ("lists_all", "lists_no_empty"):
            fn(build(n), model(n))
        return ["lists_all", "lists_no_empty"]
    return run


@_both_lists
def _e_lists_dups(b, m):
    me, k = b["meta"], b["k"]
    r = b["reads"][me["dups"]]
    km, pos = m["lists"][me["dups"]]
    for d, times in zip(me["d"], me["times"]):
        fw, rc = find_all(r, d), find_all(r, rc_bases(d))
        assert len(fw) + len(rc) == times and fw and rc
        x = canon(bases_kmer(d), k)
        assert [int(p) for p, y in zip(pos, km) if int(y) == x] == [min(fw + rc)]


@_both_lists
def _e_lists_trips(b, m):
    me = b["meta"]
    late, long3 = m["lists"][me["late"]][1], m["lists"][me["long3"]][1]
    assert len(b["reads"][me["late"]]) > 2048 and len(late) > 0 and late.min() >= 2048
    assert len(b["reads"][me["long3"]]) > 4096 and (long3 < 2048).any() and ((long3 >= 2048) & (long3 < 4096)).any() and (long3 >= 4096).any()


def _e_lists_interleaved():
    b, m = build("lists_all"), model("lists_all")
    me = b["meta"]
    n = len(b["reads"])
    for i in me["empty"] + [me["short"], me["nread"]] + me["nohit"]:
        assert len(m["lists"][i][0]) == 0
    assert len(b["reads"][me["short"]]) == b["k"] - 1 and (b["reads"][me["nread"]] > 3).any() and all(len(b["reads"][i]) == 0 for i in me["empty"])
    assert all(len(b["reads"][i]) >= 100 for i in me["nohit"])
    assert all(len(m["lists"][i][0]) > 0 for i in me["full"])
    assert len(m["lists"][0][0]) == 0 and len(m["lists"][n - 1][0]) == 0 and me["empty"][0] == 0 and me["nohit"][-1] == n - 1
    return ["lists_all"]


def _e_cap(P_of):
    def check():
        held = []
        for n in [c["name"] for c in CASES if c["kind"] == "cap" and P_of(c["P"], c["cs"])]:
            b, m = build(n), model(n)
            me, cap, P = b["meta"], b["cap"], b["P"]
            hold_ids = list(range(P, P + cap + 1))                 # reference ids of the holders, in order
            for mm, x in me["x"].items():
                lst = m["index"][canon(x, b["k"])]
                exp = list(range(P)) + hold_ids[:max(0, min(mm, cap - P))]
                assert lst == exp, (n, mm, lst, exp)
                # the reader of the unit votes for exactly those with all the unit's k-mers (k-mers that run from the unit into a spacer
                # may add votes, also for a holder whose entry was dropped: fewer than the unit has k-mers)
                nb = neighbours_of(n, me["readers"][mm])
                assert {r for r, v in nb.items() if v >= 4} == set(exp) and set(exp) <= set(m["cands"][me["readers"][mm]][0]), (n, mm)
            # between the accepted holders: a read that is not accepted and a read with N, neither in any list
            assert not b["accept"][P + 2] and (b["reads"][P + 3] > 3).any() and b["accept"][P] and b["accept"][P + 4]
            assert m["n_refs"] == P + cap + 1 + 2
            held.append(n)
        return held
    return check


def _e_cap_later_only():
    held = []
    for n in [c["name"] for c in CASES if c["kind"] == "cap"]:
        b, m = build(n), model(n)
        me = b["meta"]
        lst = m["index"][canon(me["v"], b["k"])]
        assert lst == [b["P"] + b["cap"]] and m["cands"][me["rv"]][0] == lst         # the last holder, which only the last reader shares
        for i in range(me["rv"]):
            assert lst[0] not in m["cands"][i][0] or i in me["readers"].values()
        held.append(n)
    return held


def _e_chunks():
    held = []
    for n in GRAPH_CASES:
        b, m = build(n), model(n)
        for parts, cut in b["meta"]["chunks"].items():
            assert len(cut) == parts + 1 and cut[0] == 0 and cut[-1] == len(b["reads"]) and all(x < y for x, y in zip(cut, cut[1:]))
        if b["kind"] != "cap":
            continue
        cut = b["meta"]["chunks"][5]
        acc = [bool(b["accept"][i]) and not (b["reads"][i] > 3).any() for i in range(len(b["reads"]))]
        no_ref = [j for j in range(5) if not any(acc[cut[j]:cut[j + 1]])]
        empty = [j for j in range(5) if all(len(m["lists"][i][0]) == 0 for i in range(cut[j], cut[j + 1]))]
        assert no_ref and empty and any(any(len(m["lists"][i][0]) for i in range(cut[j], cut[j + 1])) for j in no_ref), n
        held.append(n)
    return held


def _e_votes_tie():
    b, m = build("votes_c3"), model("votes_c3")
    q = b["meta"]["queries"]
    assert neighbours_of("votes_c3", q[0]) == {2: 3, 0: 2, 1: 2, 3: 2} and m["cands"][q[0]][:2] == ([2, 0, 1], [3, 2, 2])
    assert neighbours_of("votes_c3", q[1]) == {0: 1, 1: 2, 3: 1} and m["cands"][q[1]][0] == [1, 0, 3]
    return ["votes_c3"]


def _e_votes_ones():
    held = []
    for n in ("votes_c3", "votes_c1"):
        b, m = build(n), model(n)
        q = b["meta"]["queries"][2]
        assert neighbours_of(n, q) == {0: 1, 1: 1, 2: 1, 3: 1} and m["cands"][q][0] == [0, 1, 2][:b["c"]]
        held.append(n)
    return held


def _e_votes_c1():
    b, m = build("votes_c1"), model("votes_c1")
    assert b["c"] == 1 and [m["cands"][q][0] for q in b["meta"]["queries"]] == [[2], [1], [0], [1]]
    return ["votes_c1"]


def _e_votes_few():
    held = []
    for n in ("votes_c3", "hifi_common"):
        b, m = build(n), model(n)
        q = b["meta"]["queries"][3] if n == "votes_c3" else b["meta"]["q_few"]
        assert 0 < len(neighbours_of(n, q)) < b["c"] and len(m["cands"][q][0]) == len(neighbours_of(n, q))
        held.append(n)
    return held


def _e_votes_wide():
    b, m = build("votes_wide"), model("votes_wide")
    for q, want, place in ((b["meta"]["q70"], 70, 65), (b["meta"]["q140"], 140, 130)):
        nb = neighbours_of("votes_wide", q)
        assert len(nb) == want and m["cands"][q][0][0] == sorted(nb)[place - 1] and m["cands"][q][1][0] == 3
        assert sorted(nb.values())[-2] < 3
    nb = neighbours_of("votes_wide", b["meta"]["q140"])
    assert m["cands"][b["meta"]["q140"]][1][1] == 2 and sorted(nb).index(m["cands"][b["meta"]["q140"]][0][1]) >= 64      # the second one too at a stride position
    return ["votes_wide"]


def _e_hifi():
    b, m = build("hifi_common"), model("hifi_common")
    me, k = b["meta"], b["k"]
    w, z = set(_unit_kmers(me["w"], k)), set(_unit_kmers(me["z"], k))
    refs, votes, common = m["cands"][me["q"]]
    common = [common[refs.index(r)] for r in range(4)]          # (k-mers that run from a unit into a spacer may add a vote or two)
    assert sorted(refs) == [0, 1, 2, 3] and len(refs) == b["c"] and min(votes) >= len(z)
    own = {int(x) for x in m["lists"][me["q"]][0]}
    assert w <= own and w <= {int(x) for x in m["lists"][me["dropped"]][0]}        # both reads hold W ...
    assert all(me["dropped"] not in m["index"][x] for x in w)                       # ... whose entry for that read the cap dropped
    assert z <= set(common[3]) and not (w & set(common[3])) and all(w <= set(cm) for cm in common[:3])
    order = [int(x) for x in m["lists"][me["q"]][0]]
    assert all(cm == [x for x in order if x in set(cm)] for cm in common)          # in read order: Z stands before W in the query
    assert order.index(min(z, key=order.index)) < order.index(min(w, key=order.index))
    few = m["cands"][me["q_few"]]
    assert 0 < len(few[0]) < b["c"] and all(z <= set(cm) for cm in few[2])
    return ["hifi_common"]


EDGES = {
    "scan: a marker k-mer at every start offset p mod 32": _e_scan_marker_offsets,
    "scan: read lengths 0, k-1, k, k+1 and len % 32 in {0, 1, 31}": _e_scan_lengths,
    "scan: N at base 0, at the last base, at bases 31 and 32, two N a window apart; windows of reads with N counted, their lists empty": _e_scan_n,
    "modulo: the highest multiples of f below 2^64 whose preimages are canonical 28-mers survive": _e_mod("multiples"),
    "modulo: the highest multiple of an odd f itself, whose quotient equals the limit of the divide-free test": _e_mod_lim,
    "modulo: the highest hashes of the residues 1 and f-1 do not": _e_mod("near"),
    "modulo: f = 2^s d: divisible by 2^s and not by d, by d and not by 2^s": _e_mod("partial"),
    "count: units counted ci-1, ci, cs-1, cs, cs+1, 3cs": _e_count_units,
    "count: cs+1 occurrences in cs-1 distinct reads": _e_count_repeated,
    "count: key 0 from poly-A and poly-T": _e_count_poly,
    "count: the largest canonical 28-mer is the last run, of length 1": _e_count_last_single,
    "count: an input of one k-mer": _e_count_one_kmer,
    "count: an input that is one run": _e_count_one_run,
    "count: k = 6, shift 0 of the key ranges": _e_count_k6,
    "table: 13 keys of bucket 15 wrap into buckets 0, 1, 2 with keys of their own": _e_table("table_wrap", _t_wrap),
    "table: exactly 4 keys in a bucket": _e_table("table_4", _t_4),
    "table: exactly 5 keys in a bucket, the next bucket full": _e_table("table_5", _t_5),
    "table: n = 0": _e_table("table_n0", _t_n(0, 16)),
    "table: n = 1": _e_table("table_n1", _t_n(1, 16)),
    "table: n = 32 fills half of 16 buckets": _e_table("table_n32", _t_n(32, 16)),
    "table: n = 33 doubles the table": _e_table("table_n33", _t_n(33, 32)),
    "table: keys 0 and 2^56-1": _e_table("table_extremes", _t_extremes),
    "table: ranks of real canonical k-mers of a wrapping set": _e_table_ranks,
    "lists: a k-mer 2, 3 and 65 times in a read, in both orientations": _e_lists_dups,
    "lists: hits only beyond base 2048; hits in all three 64-word trips of a read over 4096 bases": _e_lists_trips,
    "lists: reads with no hit, shorter than k, with N and empty between full ones, first and last": _e_lists_interleaved,
    "cap: a k-mer in cap-1, cap, cap+1 accepted reads, no pseudo reads": _e_cap(lambda P, cap: P == 0),
    "cap: cap-1 pseudo reads in front": _e_cap(lambda P, cap: P == cap - 1),
    "cap: cap pseudo reads in front": _e_cap(lambda P, cap: P == cap),
    "cap: cap+1 pseudo reads in front": _e_cap(lambda P, cap: P == cap + 1),
    "cap: a neighbour that only later reads share": _e_cap_later_only,
    "chunks: cuts into 2 and 5, a chunk without a reference read and a chunk of empty lists": _e_chunks,
    "votes: c and c+1 neighbours, a tie across the c-th place": _e_votes_tie,
    "votes: all votes 1": _e_votes_ones,
    "votes: c = 1": _e_votes_c1,
    "votes: fewer neighbours than c": _e_votes_few,
    "votes: 70 and 140 neighbours, the winners 65th and 130th by id": _e_votes_wide,
    "hifi: shared k-mers in read order, none through an entry the cap dropped, reads with fewer than c candidates": _e_hifi,
}


def check_edges() -> dict:
    return {edge: fn() for edge, fn in EDGES.items()}
