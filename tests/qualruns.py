"""Constructed read sets that put one context run of the quality coder on every special-cased number of its kernels (k_qual_symbols,
wave_ctx_lower_bound, k_evolve_small<2|4|5>, k_evolve_large and the part layout of the interval coder in csrc/qual.hip).

Three things live here, none of which uses the code under test:
  * deterministic, seeded builders of the cases (CASES): bases, qualities, class letters (levels 2 and 3), calls and parts;
  * the context recurrence of the reference's quality coder (quality_coder_impl.cpp:78-450) over whole parts at once, and the
    adaptive counter model (one per symbol at the start, + ADDER, halve rounding up when the total reaches MAX_TOTAL);
  * the grouping rule of a call (parts of one group share a sort and a model launch; a domain start always cuts).
model_run(case) gives, for every (family, context), its run in every group of every call: L, the total it starts from, the positions
p of its rescales with the total that caused each, and the final counters.  EDGES maps every edge DESIGN.md lists to the cases that
hold it; check_edges() asserts each.  The threshold numbers (32 768, 32 765, 32 736, 16 384) are never written here: the builders
ask the counter model for them (first_rescale, epoch_after).

A context is named as cl_qual_coder_model / orc_qual_model take it (include/colord_hip.h): history fields, bases, flag bits.

What the coders must produce is not computed here: tests/golden/qualruns/cases.json records the parts of the unmodified reference
coder (oracle/ref_harness/ref_qual.cpp, tests/golden/make_qualruns.py)."""
from __future__ import annotations
import functools
import hashlib
import json
import os
import struct
import numpy as np

ORG, AVG5, AVG4, AVG2, FIX5, FIX4, FIX2, AVG, NONE = range(9)                  # QualityComprMode (params.h:33-43)
MODE_NAMES = ("org", "5-avg", "4-avg", "2-avg", "5-fix", "4-fix", "2-fix", "avg", "none")
DEFAULT_T = {AVG5: (7, 14, 26, 93), AVG4: (7, 14, 26), AVG2: (7,), FIX5: (7, 14, 26, 93), FIX4: (7, 14, 26), FIX2: (7,)}
DEFAULT_D = {FIX5: (3, 10, 18, 35, 93), FIX4: (3, 10, 18, 35), FIX2: (1, 13)}
BYTE_MODEL = (256, 1 << 18, 8)                                                 # quality_coder.h:41
DEFAULT_GROUP_SYMS = (1 << 31) - (1 << 24)                                     # qual.hip: GROUP_SYMS
# quantisation of the history in org mode: class bounds by (source is ONT, level is 3) (quality_coder.cpp:276-504)
_QUANT = {(True, True): (0, 1, 2, 4, 7, 11, 16, 22, 29, 37, 46, 56, 67, 79, 90, 96), (True, False): (0, 1, 2, 5, 10, 15, 20, 25, 35, 50, 70, 96),
          (False, True): (0, 1, 10, 20, 30, 39, 45, 51, 57, 63, 69, 75, 81, 87, 93, 94), (False, False): (0, 1, 15, 29, 41, 53, 63, 72, 80, 87, 93, 94)}


def cfg_of(c: dict) -> dict:
    """the coder's tables for a case (CQualityCoder::Init, quality_coder.cpp:26-270)"""
    mode, level, source = c["mode"], c["level"], c.get("source", 0)
    g = dict(mode=mode, level=level, source=source, per_base=mode <= FIX2, is_avg=mode in (AVG5, AVG4, AVG2))
    if mode == ORG:
        g.update(n_sym=96, n_fields=2, max_total=1 << 20, adder=32, n_bins=0)   # quality_coder.h:36
        g["map_fwd"] = np.arange(96, dtype=np.int64)
        q = np.zeros(96, np.int64)
        t = _QUANT[(source == 0, level == 3)]
        for b in range(len(t) - 1):
            q[t[b]:t[b + 1]] = b
        if source == 2:
            q[:93] += 1; q[93] = 0
        g["quant"] = q
    elif mode <= FIX2:
        n = {AVG5: 5, FIX5: 5, AVG4: 4, FIX4: 4, AVG2: 2, FIX2: 2}[mode]
        g.update(n_sym=n, n_fields=6 if n == 2 else 3, max_total=1 << 18, adder=8, n_bins=n)   # :37-39
        T = tuple(c.get("fwd") or DEFAULT_T[mode])
        assert len(T) == n - 1 and all(a <= b for a, b in zip(T, T[1:])) and T[-1] <= 96
        m = np.zeros(96, np.int64)                                              # adjust_quality_map_symbols (quality_coder.cpp:250-270)
        for b in range(1, n - 1):
            m[T[b - 1]:T[b]] = b
        m[T[-1]:] = n - 1
        g["map_fwd"] = m
        g["T"] = T
    else:
        g.update(n_sym=2, n_fields=0, max_total=1 << 18, adder=8, n_bins=0)
    g["navg"] = {AVG5: 10, AVG4: 8, AVG2: 4, AVG: 2}.get(mode, 0)
    return g


# ---- the adaptive counter model (rc.h:233-244 of the reference) ------------------------------------------------------------
def evolve(counts: np.ndarray, syms: np.ndarray, max_total: int, adder: int):
    """Feeds syms to the counters in place.  Returns [(p, total)]: a rescale happened when p symbols of syms were consumed
    (1 <= p <= len(syms)), caused by the total `total` (>= max_total)."""
    n, pos, out = len(counts), 0, []
    syms = np.asarray(syms, np.int64)
    while True:
        tot = int(counts.sum())
        rr = -(-(max_total - tot) // adder)                    # symbols until the total reaches MAX_TOTAL
        if pos + rr > len(syms):
            counts += adder * np.bincount(syms[pos:], minlength=n)
            return out
        counts += adder * np.bincount(syms[pos:pos + rr], minlength=n)
        pos += rr
        out.append((pos, int(counts.sum())))
        while int(counts.sum()) >= max_total:
            counts[:] = (counts + 1) // 2


def evolve_one_by_one(counts: np.ndarray, syms, max_total: int, adder: int):
    """The same, a symbol at a time as the reference's model does it: the check of evolve()."""
    out = []
    for i, s in enumerate(syms):
        counts[s] += adder
        if int(counts.sum()) >= max_total:
            out.append((i + 1, int(counts.sum())))
            while int(counts.sum()) >= max_total:
                counts[:] = (counts + 1) // 2
    return out


def first_rescale(n_sym: int, max_total: int, adder: int) -> int:
    """symbols a fresh model takes until its first rescale (asked of the model, never written down)"""
    return evolve(np.ones(n_sym, np.int64), np.zeros(max_total, np.int64), max_total, adder)[0][0]


def epoch_after(n_sym: int, max_total: int, adder: int, k: int = 1) -> int:
    """symbols between rescale k and rescale k + 1 of a run of one repeated symbol"""
    r = evolve(np.ones(n_sym, np.int64), np.zeros(max_total * (k + 1), np.int64), max_total, adder)
    return r[k][0] - r[k - 1][0]


# ---- the context recurrence over a whole part ---------------------------------------------------------------------------
def api_context(fields, b0=0, bm1=0, bm2=0, bp1=0, later=0, fl=0) -> int:
    """a per-base context as cl_qual_coder_model takes it: fields = the history, the position before first, 0xF = no such position"""
    v = 0
    for t, f in enumerate(fields):
        v |= int(f) << (4 * t)
    return v | (b0 << 32) | (bm1 << 34) | (bm2 << 36) | (bp1 << 38) | (later << 40) | (fl << 48)


def _base_ctx(g, b0, bm1, bm2, bp1, later):
    """the neighbouring-base part of a context as the reference lays it out (quality_coder_impl.cpp:88-108, 159-172, 323-339)"""
    if g["is_avg"]:
        return (bm2 << 6) | (bm1 << 4) | (b0 << 2) | bp1
    if g["mode"] != ORG or g["level"] == 3:
        return b0 | (bm1 << 2) | (bm2 << 4) | (bp1 << 6)
    return b0 | (bm1 << 2) | ((later & (bm2 == bm1)).astype(np.int64) << 4) | (bp1 << 5)


def model_key(g, api) -> int:
    """the identity of the reference's model behind an api context: what the level-1/2 org context forgets about bm2 is forgotten"""
    api = np.atleast_1d(np.asarray(api, dtype=np.int64))
    bc = _base_ctx(g, (api >> 32) & 3, (api >> 34) & 3, (api >> 36) & 3, (api >> 38) & 3, (api >> 40) & 1)
    k = (api & 0xffffff) | (bc << 24) | (((api >> 48) & 3) << 32)
    return k


def part_symbols(g, bases, quals, flags, off):
    """Per-base (api context, model key, symbol) of every base of the reads [off[0], off[-1]) of one part, in stream order, and the
    byte-family (context, symbol) pairs with the per-read bin sums and counts they come from."""
    lo, hi = int(off[0]), int(off[-1])
    n_reads = len(off) - 1
    lens = np.diff(off).astype(np.int64)
    rid = np.repeat(np.arange(n_reads), lens)
    pos = np.arange(lo, hi, dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), lens)
    rlen = np.repeat(lens, lens)
    q = quals[lo:hi].astype(np.int64) - 33
    out = dict(api=np.zeros(0, np.int64), key=np.zeros(0, np.int64), sym=np.zeros(0, np.int64), bctx=np.zeros(0, np.int64), bsym=np.zeros(0, np.int64))
    if g["mode"] == NONE:
        return out
    assert q.min(initial=0) >= 0 and q.max(initial=0) <= (94 if g["mode"] != ORG or g["source"] == 0 else 93), "a quality value the reference's tables do not cover"
    if g["mode"] == AVG:                                       # quality_coder_impl.cpp:438-450
        s = np.bincount(rid, weights=q, minlength=n_reads).astype(np.int64)
        a = (s.astype(np.float64) / lens.astype(np.float64) * 256).astype(np.int64)
        out["bctx"] = np.stack([np.zeros(n_reads, np.int64), 640 + (a >> 8)], 1).ravel()
        out["bsym"] = np.stack([a >> 8, a & 255], 1).ravel()
        out["sums"], out["cnts"] = s[:, None], lens[:, None]
        return out
    sym = g["map_fwd"][q]
    if g["is_avg"]:                                            # :138-157
        nb = g["n_bins"]
        s = np.bincount(rid * nb + sym, weights=q, minlength=n_reads * nb).astype(np.int64).reshape(n_reads, nb)
        cn = np.bincount(rid * nb + sym, minlength=n_reads * nb).astype(np.int64).reshape(n_reads, nb)
        avg = np.where(cn > 0, s.astype(np.float64) / np.maximum(cn, 1).astype(np.float64), 0.0)
        a = (avg * 256).astype(np.int64)
        ctx_p = np.concatenate([np.zeros((n_reads, 1), np.int64), avg.astype(np.int64)[:, :-1]], 1)
        hi_ctx = np.arange(nb)[None, :] * 128 + ctx_p
        out["bctx"] = np.stack([hi_ctx, 640 + (a >> 8)], 2).ravel()
        out["bsym"] = np.stack([a >> 8, a & 255], 2).ravel()
        out["sums"], out["cnts"] = s, cn
    field = g["quant"][sym] if g["mode"] == ORG else sym
    api = np.zeros(hi - lo, np.int64)
    def back(v, d, fill):
        """v of the position d before, `fill` where the read has none"""
        w = np.full(hi - lo, fill, np.int64)
        if hi - lo > d:
            w[d:] = np.where(pos[d:] >= d, v[:-d], fill)
        return w
    for t in range(1, g["n_fields"] + 1):
        api |= back(field, t, 0xF) << (4 * (t - 1))
    vs = bases[lo:hi].astype(np.int64) & 3                     # valid_sym: N counts as A
    bm1, bm2 = back(vs, 1, 0), back(vs, 2, 0)
    bp1 = np.where(pos + 1 < rlen, np.concatenate([vs[1:], np.zeros(1, np.int64)]), 0)
    later = (pos > 1).astype(np.int64)
    fl = np.zeros(hi - lo, np.int64)
    if g["level"] > 1:
        f = flags[lo:hi]
        fl = (f == ord("M")).astype(np.int64) | ((f == ord("A")).astype(np.int64) << 1)
    api |= (vs << 32) | (bm1 << 34) | (bm2 << 36) | (bp1 << 38) | (later << 40) | (fl << 48)
    out["api"], out["sym"] = api, sym
    out["key"] = model_key(g, api)
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------
# Every case: kind (its builder), seed, mode / source / level / fwd / rev, what the kind needs, `targets`.  Numbers that depend on the
# counter model are expressions over: first / epoch (the per-base family's first rescale and the epoch after it), bfirst (the byte
# family's first rescale), n (the mode's history fields).
def _hot(name, mode, hot, calls, **kw):
    d = dict(name=name, kind="hot", mode=mode, level=1, hot=hot, calls=calls, base=1, gap=[kw.pop("gap_lo", 0), kw.pop("gap_hi", 0)], targets=[["pos", 0, "n"]])
    d.update(kw)
    return d


_SMALL = {2: (FIX2, [3], [12], 7, 14), 4: (AVG4, [9], [30], 4, 9), 5: (FIX5, [20], [95 - 1], 4, 9)}   # alphabet: mode, pool, spot, gaps
_P_OF_R = {1: 193, 63: 191, 64: 128, 65: 65}                                   # the p (symbols of the second call at the rescale) that leaves r updates at a step's start
CASES = []
for _a, (_m, _pool, _spot, _g0, _g1) in _SMALL.items():
    for _r, _p in _P_OF_R.items():
        CASES.append(_hot(f"small{_a}_r{_r}", _m, [f"first-{_p}", f"{_p}+100"], [[0, 1], [1, 2]], pool=_pool, spot=_spot, gap_lo=_g0, gap_hi=_g1, seed=100 + 10 * _a + _r % 7, r_left=_r))
CASES += [
    _hot("small4_rescale_on_last", AVG4, ["first-300", "300"], [[0, 1], [1, 2]], pool=[9], spot=[30], gap_lo=4, gap_hi=9, seed=201),
    _hot("small4_one_short", AVG4, ["first-1", "70"], [[0, 1], [1, 2]], pool=[9], spot=[30], gap_lo=4, gap_hi=9, seed=202),
    _hot("small2_step_of_64_equal", FIX2, ["64"], [[0, 1]], pool=[3], spot=[], seed=203),
    _hot("small4_two_rescales", AVG4, ["first+epoch+100"], [[0, 1]], pool=[9, 10, 12], spot=[30], gap_lo=30, gap_hi=60, seed=204),
    _hot("org_l1_mid_step", ORG, ["first+200"], [[0, 1]], pool=[10, 11, 12, 13, 14], spot=[40], gap_lo=8, gap_hi=20, seed=301),
    _hot("org_l1_split_step_bound", ORG, ["first-128", "128+90"], [[0, 1], [1, 2]], pool=[10, 11, 12, 13, 14], spot=[0], gap_lo=8, gap_hi=20, seed=302),
    _hot("org_hifi_l1", ORG, ["first-61", "61+70"], [[0, 1], [1, 2]], source=2, pool=[93], spot=[0, 50], gap_lo=5, gap_hi=12, seed=303),
    _hot("org_l2_match", ORG, ["first+70"], [[0, 1]], level=2, flag="M", pool=[10, 11, 12, 13, 14], spot=[94], gap_lo=8, gap_hi=20, seed=304),
    _hot("org_pb_l3_anchor", ORG, ["first+70"], [[0, 1]], source=1, level=3, flag="A", base=3, pool=[20, 23, 29], spot=[93], gap_lo=8, gap_hi=20, seed=305),
    dict(name="byte_avg", kind="short_reads", mode=AVG, level=1, seed=401, n_reads="bfirst+64", lens=[1, 3], calls=[[0, "bfirst+64"]],
         targets=[["byte", 0], ["byte", 640 + 10], ["byte", 640 + 94], ["byte", 640 + 95]]),
    dict(name="byte_avg2", kind="short_reads", mode=AVG2, level=1, seed=402, n_reads="bfirst+40", lens=[1, 1], calls=[[0, "bfirst-8", "bfirst+40"]],
         targets=[["byte", 0], ["byte", 128], ["byte", 128 + 3], ["byte", 128 + 6], ["byte", 640], ["byte", 640 + 20], ["pos", 0, 0]]),
    dict(name="averages", kind="averages", mode=AVG5, level=1, fwd=[2, 9, 30, 94], seed=403, calls=[[0, 3, 6, 36]],
         targets=[["byte", 0], ["byte", 128], ["byte", 4 * 128 + 93], ["byte", 640], ["byte", 640 + 93], ["pos", 4, 5]]),
]
for _n in (1, 63, 64, 65, 4096, 4097):
    CASES.append(dict(name=f"lb_whole_{_n}", kind="lb_whole", mode=FIX2, level=1, seed=500 + _n % 50, n=_n, calls=[[0, _n]], targets=["all"]))
    CASES.append(dict(name=f"lb_mixed_fix2_{_n}", kind="lb_mixed", mode=FIX2, level=1, seed=520 + _n % 50, n=_n, targets=["all"]))
    CASES.append(dict(name=f"lb_mixed_avg4_{_n}", kind="lb_mixed", mode=AVG4, level=2, seed=540 + _n % 50, n=_n, targets=["all"]))
_BOUND_LENS = [1, 2, 3, 4, 5, 6, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129]
for _nm, _kw in (("org_l1", dict(mode=ORG, level=1)), ("org_l2", dict(mode=ORG, level=2)), ("org_hifi_l3", dict(mode=ORG, level=3, source=2)),
                 ("fix2_l1", dict(mode=FIX2, level=1)), ("avg4_l3", dict(mode=AVG4, level=3)), ("avg5_l2", dict(mode=AVG5, level=2))):
    CASES.append(dict(name=f"bounds_{_nm}", kind="bounds", seed=600 + len(CASES), targets=["all"], **_kw))
for _nm, _np, _order, _empty in (("1_equal", 1, "equal", []), ("63_desc", 63, "desc", []), ("64_asc", 64, "asc", []), ("64_equal", 64, "equal", []),
                                 ("65_equal_empties", 65, "equal", [0, 32, 64]), ("129_desc_empties", 129, "desc", [0, 64, 65, 128]), ("129_asc", 129, "asc", [])):
    CASES.append(dict(name=f"parts_{_nm}", kind="parts", mode=AVG4, level=1, seed=700 + _np, n_parts=_np, order=_order, empty=_empty,
                      targets=[["pos", 0, 0], ["byte", 0], ["byte", 640 + 9]]))
CASES += [
    dict(name="thr_avg2_custom", kind="random", mode=AVG2, level=1, fwd=[20], seed=801, n_reads=60, targets=[["pos", 3, 0], ["byte", 0]]),
    dict(name="thr_fix4_custom", kind="random", mode=FIX4, level=2, fwd=[3, 40, 94], rev=[1, 20, 60, 94], seed=802, n_reads=60, targets=[["pos", 3, 0]]),
    dict(name="thr_fix5_custom", kind="random", mode=FIX5, level=1, fwd=[1, 2, 50, 95], rev=[0, 1, 20, 60, 95], seed=803, n_reads=60, targets=[["pos", 3, 0]]),
    dict(name="thr_avg4_equal", kind="random", mode=AVG4, level=1, fwd=[7, 7, 26], seed=804, n_reads=60, targets=[["pos", 3, 0], ["byte", 128], ["byte", 2 * 128]]),
    # one hot run over four parts of one call; with group_syms the call is cut into two groups of two parts, the rescale in the second
    dict(name="groups_avg4", kind="hot", mode=AVG4, level=1, hot=["first//2-100", "first//2-100", "150", "150"], calls=[[0, 1, 2, 3, 4]], base=2, gap=[4, 9], pool=[9], spot=[30],
         seed=901, group_syms="2 parts", groups=2, targets=[["pos", 0, "n"], ["byte", 0]]),
    dict(name="groups_avg4_domains", kind="hot", mode=AVG4, level=1, hot=["first//2-100", "first//2-100", "150", "150"], calls=[[0, 1, 2, 3, 4]], base=2, gap=[4, 9], pool=[9], spot=[30],
         seed=901, group_syms="2 parts", groups=2, domain_symbols="2 parts", targets=[["pos", 0, "n"], ["byte", 0]]),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def numbers(c: dict) -> dict:
    g = cfg_of(c)
    d = dict(n=g["n_fields"], bfirst=first_rescale(*BYTE_MODEL))
    if g["per_base"]:
        d.update(first=_first(g["n_sym"], g["max_total"], g["adder"]), epoch=_epoch(g["n_sym"], g["max_total"], g["adder"]))
    return d


@functools.lru_cache(maxsize=None)
def _first(n, mt, ad):
    return first_rescale(n, mt, ad)


@functools.lru_cache(maxsize=None)
def _epoch(n, mt, ad):
    return epoch_after(n, mt, ad)


def _num(c, x):
    return x if isinstance(x, int) else int(eval(x, {"__builtins__": {}}, numbers(c)))


def _letters(rng, length, level):
    """class letters of one read at levels 2 and 3: a plain read, or runs of anchor / match / other"""
    if level <= 1:
        return np.full(length, ord("P"), np.uint8)
    if rng.random() < 0.25:
        return np.full(length, ord("P"), np.uint8)
    out = np.zeros(length, np.uint8)
    i = 0
    while i < length:
        k = int(rng.integers(1, 9))
        out[i:i + k] = rng.choice(np.frombuffer(b"AM ", np.uint8))
        i += k
    return out


def _max_q(c):
    return 94 if c["mode"] != ORG or c.get("source", 0) == 0 else 93


def _random_read(rng, c, length, n_at=()):
    b = rng.integers(0, 4, length).astype(np.uint8)
    for p in n_at:
        if 0 <= p < length:
            b[p] = 4
    q = rng.integers(0, _max_q(c) + 1, length)
    edge = rng.random(length) < 0.15                            # the ends of the alphabet often
    q[edge] = rng.choice([0, 1, _max_q(c) - 1, _max_q(c)], int(edge.sum()))
    return b, (q + 33).astype(np.uint8), _letters(rng, length, c["level"])


def _hot_read(rng, c, g, n_hot):
    """a homopolymer whose qualities keep one history (values of `pool`, one class / bin) but for `spot` values at random gaps, cut so
    that exactly n_hot positions lie in the context of its position n (every field the pool's, every base the read's)"""
    n = g["n_fields"]
    lo, hi = c["gap"]
    mean = (lo + hi) / 2
    length = n + 2 + (int(n_hot * mean / (mean - n) * 1.25) if c["spot"] else n_hot) + 4 * (hi + n + 2)
    q = rng.choice(c["pool"], length)
    if c["spot"]:
        at = n + 1 + np.cumsum(rng.integers(lo, hi + 1, length // lo + 1))
        at = at[at < length]
        q[at] = rng.choice(c["spot"], len(at))
    b = np.full(length, c["base"], np.uint8)
    f = np.full(length, ord(c.get("flag", "P")), np.uint8)
    s = part_symbols(g, b, (q + 33).astype(np.uint8), f, np.array([0, length]))
    is_hot = s["key"] == s["key"][n]
    is_hot[-1] = False
    cut = int(np.searchsorted(np.cumsum(is_hot), n_hot)) + 2   # the n_hot-th hot position is the last but one
    assert cut <= length - 1 and int(is_hot[:cut - 1].sum()) == n_hot
    return b[:cut], (q[:cut] + 33).astype(np.uint8), f[:cut]


@functools.lru_cache(maxsize=None)
def build(name: str) -> dict:
    """dict(bases, quals, flags (class letters, every level), off, calls = [[read bounds of the parts of a call]], cfg)"""
    c = BY_NAME[name]
    g = cfg_of(c)
    rng = np.random.default_rng(c["seed"])
    kind, reads, calls = c["kind"], [], None
    if kind == "hot":
        reads = [_hot_read(rng, c, g, _num(c, h)) for h in c["hot"]]
    elif kind == "short_reads":
        for _ in range(_num(c, c["n_reads"])):
            reads.append(_random_read(rng, c, int(rng.integers(c["lens"][0], c["lens"][1] + 1))))
    elif kind == "averages":
        T = c["fwd"]
        bins = [list(range(0, T[0]))] + [list(range(T[i], T[i + 1])) for i in range(3)] + [[94]]
        pick = lambda b, k: rng.choice(bins[b], k)
        qs = [np.concatenate([pick(0, 25), pick(4, 15)]),                       # bins 1-3 empty
              np.full(17, 20),                                                  # one bin, an integral average
              np.concatenate([pick(1, 3), np.full(5, 93), pick(4, 1)]),         # count 3; the bin before the last averages 93
              np.concatenate([pick(2, 7), pick(3, 255), pick(0, 257)]),         # counts 7, 255, 257
              np.concatenate([np.full(6, 4), np.full(6, 12), np.full(6, 30)]),  # three integral averages
              np.concatenate([pick(3, 3), pick(2, 255)])]
        qs = [rng.permutation(q) for q in qs]
        for q in qs:
            reads.append((rng.integers(0, 4, len(q)).astype(np.uint8), (q + 33).astype(np.uint8), np.full(len(q), ord("P"), np.uint8)))
        reads += [_random_read(rng, c, int(rng.integers(1, 300))) for _ in range(30)]
    elif kind == "lb_whole":
        for _ in range(c["n"]):
            b, q, f = _random_read(rng, c, 1)
            reads.append((np.full(1, 2, np.uint8), q, f))
        calls = [[0, c["n"]]]
    elif kind == "lb_mixed":
        left = c["n"]
        top = 33 + 94
        if left >= 63:                                          # every component 0, and every component at its largest reachable value
            k = g["n_fields"] + 5
            reads.append((np.zeros(k, np.uint8), np.full(k, 33, np.uint8), np.full(k, ord(" "), np.uint8)))
            reads.append((np.full(k, 3, np.uint8), np.full(k, top, np.uint8), np.full(k, ord("A" if c["level"] > 1 else "P"), np.uint8)))
            left -= 2 * k
        while left:
            k = min(left, int(rng.integers(1, 40)))
            reads.append(_random_read(rng, c, k)); left -= k
        order = rng.permutation(len(reads))
        reads = [reads[i] for i in order]
        calls = [[0, len(reads) // 2, len(reads)]] if len(reads) > 1 else [[0, 1]]
    elif kind == "bounds":
        for i, ln in enumerate(_BOUND_LENS):
            reads.append(_random_read(rng, c, ln, n_at=(0,) if i % 3 == 0 else (31, 32) if i % 3 == 1 else (ln - 1,)))
            reads.append(_random_read(rng, c, ln))
        for head in ([0], [0, 0], [0, 1], [1, 0], [0, 0, 0], [1, 1], [4, 0], [0, 4, 0]):    # reads that begin with A, AA, ...: position 1 and 2 of the level-1/2 org context
            b, q, f = _random_read(rng, c, 12)
            b[:len(head)] = head
            reads.append((b, q, f))
        b, q, _ = _random_read(rng, c, 40)                      # one (history, bases) under each class letter
        b[:] = 2
        q[:] = 33 + 12
        for letter in b"AM P":
            reads.append((b.copy(), q.copy(), np.full(40, letter if c["level"] > 1 else ord("P"), np.uint8)))
        calls = [[0, 7, len(reads) // 2, len(reads)]]
    elif kind == "parts":
        n_parts = c["n_parts"]
        per, bounds = [], [0]
        for p in range(n_parts):
            k = {"equal": 2, "desc": 1 + (n_parts - 1 - p) // 4, "asc": 1 + p // 4}[c["order"]]
            per.append(0 if p in c["empty"] else k)
        for k in per:
            for i in range(k):                                 # the first read of a part is one base: (no history, C, no base behind) in every part
                b, q, f = _random_read(rng, c, 1 if i == 0 else int(rng.integers(1, 4)))
                b[:] = 1
                q[0] = 33 + 9
                reads.append((b, q, f))
            bounds.append(len(reads))
        calls = [bounds]
    elif kind == "random":
        reads = [_random_read(rng, c, int(rng.integers(1, 400)), n_at=(int(rng.integers(0, 50)),)) for _ in range(c["n_reads"])]
        calls = [[0, c["n_reads"] // 3, c["n_reads"]]]
    else:
        raise AssertionError(kind)
    if calls is None:
        calls = [[_num(c, x) for x in cb] for cb in c["calls"]]
    off = np.concatenate([[0], np.cumsum([len(r[0]) for r in reads])]).astype(np.int64)
    assert all(len(r[0]) >= 1 for r in reads), "the reference reads the first base of every read"
    assert calls[0][0] == 0 and calls[-1][-1] == len(reads) and all(a[-1] == b[0] for a, b in zip(calls, calls[1:]))
    return dict(bases=np.concatenate([r[0] for r in reads]), quals=np.concatenate([r[1] for r in reads]), flags=np.concatenate([r[2] for r in reads]),
                off=off, calls=calls, cfg=g, n_reads=len(reads))


def part_bounds(b) -> list:
    """the read bounds of all parts of all calls, in order"""
    out = [0]
    for cb in b["calls"]:
        out += cb[1:]
    return out


def syms_of(b, r0: int, r1: int) -> int:
    """coded symbols of the reads [r0, r1): one a base (not avg) and the average bytes of every read"""
    g = b["cfg"]
    return (int(b["off"][r1] - b["off"][r0]) if g["per_base"] else 0) + (r1 - r0) * g["navg"]


def _two_parts(b, x):
    """'2 parts': the symbols of the first two parts of the first call"""
    if x is None or isinstance(x, int):
        return x
    assert x == "2 parts"
    return syms_of(b, 0, b["calls"][0][2])


def plan(name: str, group_syms: int | None = None):
    """[(call, [part indices of a group], the group starts a domain)] as qual_prepare cuts a call: a part opens a domain when the open
    one holds domain_symbols or more; a group takes parts while it stays within group_syms and meets no domain start"""
    c, b = BY_NAME[name], build(name)
    limit = group_syms or DEFAULT_GROUP_SYMS
    dom_n = _two_parts(b, c.get("domain_symbols")) or 0
    since, out, pi = 0, [], 0
    for ci, cb in enumerate(b["calls"]):
        n_parts = len(cb) - 1
        opens = []
        for p in range(n_parts):
            o = bool(dom_n and since >= dom_n)
            if o:
                since = 0
            opens.append(o)
            since += syms_of(b, cb[p], cb[p + 1])
        p0 = 0
        while p0 < n_parts:
            p1 = p0 + 1
            while p1 < n_parts and not opens[p1] and syms_of(b, cb[p0], cb[p1 + 1]) <= limit:
                p1 += 1
            out.append((ci, list(range(pi + p0, pi + p1)), opens[p0]))
            p0 = p1
        pi += n_parts
    return out


def group_syms_of(name: str):
    return _two_parts(build(name), BY_NAME[name].get("group_syms"))


def domain_symbols_of(name: str):
    return _two_parts(build(name), BY_NAME[name].get("domain_symbols"))


def domain_starts(name: str) -> list:
    """the first part of every model domain (what cl_qual_coder_domains must report)"""
    return [0] + [parts[0] for _, parts, opens in plan(name) if opens]


@functools.lru_cache(maxsize=None)
def model_run(name: str, group_syms: int | None = None) -> dict:
    """The counter model over the whole case.  dict(final = {(family, key): counts}, runs = {(family, key): [dict(call, group, L,
    start_total, rescales = [(p, total)])]}, api = {key: an api context of it}, parts = the per-part symbols).  p counts the symbols of
    the run inside its group: the kernels take a run 64 symbols a step from the start of the group's run."""
    b = build(name)
    g = b["cfg"]
    pb = part_bounds(b)
    parts = [part_symbols(g, b["bases"], b["quals"], b["flags"], b["off"][pb[p]:pb[p + 1] + 1]) if pb[p + 1] > pb[p] else None for p in range(len(pb) - 1)]
    state, runs, api = {}, {}, {}
    for gi, (call, plist, opens) in enumerate(plan(name, group_syms)):
        if opens:
            state = {}
        for fam, kf, sf, (n, mt, ad) in ((0, "key", "sym", (g["n_sym"], g["max_total"], g["adder"])), (1, "bctx", "bsym", BYTE_MODEL)):
            ps = [parts[p] for p in plist if parts[p] is not None]
            if not ps:
                continue
            keys = np.concatenate([p[kf] for p in ps]); syms = np.concatenate([p[sf] for p in ps])
            if not len(keys):
                continue
            order = np.argsort(keys, kind="stable")
            ks, ss = keys[order], syms[order]
            cut = np.flatnonzero(np.diff(ks)) + 1
            if fam == 0:
                apis = np.concatenate([p["api"] for p in ps])[order]
            for s, e in zip(np.concatenate([[0], cut]), np.concatenate([cut, [len(ks)]])):
                k = (fam, int(ks[s]))
                counts = state.setdefault(k, np.ones(n, np.int64))
                start = int(counts.sum())
                res = evolve(counts, ss[s:e], mt, ad)
                runs.setdefault(k, []).append(dict(call=call, group=gi, L=int(e - s), start_total=start, rescales=res))
                if fam == 0:
                    api.setdefault(k[1], int(apis[s]))
    return dict(final=state, runs=runs, api=api, parts=parts)


def all_targets(name: str) -> list:
    """[(family, api context)] of the case's targeted models, and for a case that targets "all" every per-base context it codes plus
    three it never does"""
    c, b = BY_NAME[name], build(name)
    g = b["cfg"]
    out = []
    for t in c["targets"]:
        if t == "all":
            m = model_run(name)
            out += [(0, a) for a in m["api"].values()]
            n = g["n_fields"]
            top = int(g["quant"].max()) if g["mode"] == ORG else g["n_sym"] - 1        # the largest value a history field holds
            out += [(0, a) for a in (api_context([0] * n, 1, 2, 3, 0, 1), api_context([0xF] * n, 3, 1), api_context([top] * n, 3, 3, 3, 3, 1, 2 if g["level"] > 1 else 0))]
        elif t[0] == "byte":
            out.append((1, t[1]))
        else:
            r = t[1]
            s = part_symbols(g, b["bases"], b["quals"], b["flags"], b["off"][r:r + 2])
            out.append((0, int(s["api"][_num(c, t[2])])))
    return list(dict.fromkeys(out))


def target_key(name: str, which: int = 0):
    fam, a = all_targets(name)[which]
    return (fam, int(model_key(build(name)["cfg"], a)[0]) if fam == 0 else a)


def target_model(name: str, fam: int, a: int, group_syms=None) -> np.ndarray:
    """counters and total the model ends with for one targeted context"""
    g = build(name)["cfg"]
    k = (fam, int(model_key(g, a)[0]) if fam == 0 else a)
    n = g["n_sym"] if fam == 0 else 256
    cnt = model_run(name, group_syms)["final"].get(k, np.ones(n, np.int64))
    return np.append(cnt, cnt.sum()).astype(np.uint32)


# ---- the edges and the cases that hold them ------------------------------------------------------------------------------
def _runs(name, which=0, group_syms=None):
    return model_run(name, group_syms)["runs"].get(target_key(name, which), [])


def _mt(name, which=0):
    g = build(name)["cfg"]
    return (g["max_total"], g["adder"], g["n_sym"]) if all_targets(name)[which][0] == 0 else (BYTE_MODEL[1], BYTE_MODEL[2], 256)


def _rescales_in_call(r, call):
    return [x for run in r if run["call"] == call for x in run["rescales"]]


def _r_left(name, r):
    """the second call's run meets a rescale with r updates left at the start of a step: the steps before it are whole"""
    (p, _), = _rescales_in_call(_runs(name), 1)[:1]
    return p >= r and (p - r) % 64 == 0 and (r != 1 or p > 64) and (r != 65 or p == 65) and _runs(name)[1]["L"] > p


_SMALL_NAMES = lambda r: [f"small{a}_r{r}" for a in (2, 4, 5)]
EDGES = {
    # edge: (cases, predicate over (case name, the runs of its first target))
    "small alphabets: a rescale with 1 update left at a step's start (lane 1 splits the step)": (_SMALL_NAMES(1), lambda n, r: _r_left(n, 1)),
    "small alphabets: 63 updates left (the step's last lane starts an epoch)": (_SMALL_NAMES(63), lambda n, r: _r_left(n, 63)),
    "small alphabets: 64 updates left (now == 64, the rescale on the step's bound)": (_SMALL_NAMES(64), lambda n, r: _r_left(n, 64)),
    "small alphabets: 65 updates left (a whole step, then lane 1)": (_SMALL_NAMES(65), lambda n, r: _r_left(n, 65)),
    "the first rescale jumps past MAX_TOTAL (small alphabets)": (_SMALL_NAMES(1), lambda n, r: _rescales_in_call(r, 1)[0][1] > _mt(n)[0]),
    "a rescale on the last symbol of the run": (["small4_rescale_on_last"], lambda n, r: r[1]["rescales"] == [(r[1]["L"], r[1]["rescales"][0][1])] and r[1]["L"] % 64 != 0),
    "a call that starts one update below MAX_TOTAL (rescale at p = 1)": (["small4_one_short"], lambda n, r: r[1]["start_total"] + _mt(n)[1] >= _mt(n)[0] > r[1]["start_total"] and r[1]["rescales"][0][0] == 1),
    "one step of 64 equal symbols": (["small2_step_of_64_equal"], lambda n, r: len(r) == 1 and r[0]["L"] == 64 and _one_symbol(n)),
    "two rescales in one call": (["small4_two_rescales"], lambda n, r: len(r[0]["rescales"]) == 2 and r[0]["L"] > r[0]["rescales"][1][0]),
    "org: total == MAX_TOTAL exactly, in mid-step": (["org_l1_mid_step", "org_l2_match", "org_pb_l3_anchor"], lambda n, r: r[0]["rescales"][0][1] == _mt(n)[0] and r[0]["rescales"][0][0] % 64 not in (0, 1, 63)),
    "org: total == MAX_TOTAL exactly on a step bound of the second call": (["org_l1_split_step_bound"], lambda n, r: r[1]["rescales"][0][1] == _mt(n)[0] and r[1]["rescales"][0][0] % 64 == 0 and r[0]["rescales"] == []),
    "org, source 2: the history class 0 of value 93, the rescale in the second call": (["org_hifi_l1"], lambda n, r: (all_targets(n)[0][1] & 0xff) == 0 and r[1]["rescales"][0][1] == _mt(n)[0] and r[1]["rescales"][0][0] == 61),
    "org at levels 2 and 3: the hot context carries a flag bit": (["org_l2_match", "org_pb_l3_anchor"], lambda n, r: (all_targets(n)[0][1] >> 48) == {"org_l2_match": 1, "org_pb_l3_anchor": 2}[n]),
    "byte family: hi(0, 0) rescales with total == MAX_TOTAL exactly": (["byte_avg", "byte_avg2"], lambda n, r: _rescales_in_call(r, 0)[0][1] == BYTE_MODEL[1] and all_targets(n)[0] == (1, 0)),
    "groups: a hot run crosses a group bound that is no domain start, the rescale in the second group": (["groups_avg4"], lambda n, r: _group_edge(n, False)),
    "groups: the same cut as a domain start, the second group starts fresh": (["groups_avg4_domains"], lambda n, r: _group_edge(n, True)),
}


def _one_symbol(name):
    m = model_run(name)
    k = target_key(name)
    return int((m["final"][k] > 1).sum()) == 1


def _group_edge(name, domains):
    c = BY_NAME[name]
    gs = group_syms_of(name)
    p_unset, p_set = plan(name), plan(name, gs)
    assert len(p_set) == c["groups"] == 2 and [x[1] for x in p_set] == [[0, 1], [2, 3]]
    r = _runs(name, 0, gs)
    if domains:
        assert [x[2] for x in p_set] == [False, True] and len(p_unset) == 2 and domain_starts(name) == [0, 2]
        return len(r) == 2 and r[1]["start_total"] == _mt(name)[2] and r[1]["rescales"] == [] and r[0]["rescales"] == []
    assert [x[2] for x in p_set] == [False, False] and len(p_unset) == 1
    whole = _runs(name, 0, None)
    # one group: the rescale in mid-run; two groups: the same symbol is a rescale of the second group's run, which starts from the first's counters
    return (len(whole) == 1 and len(r) == 2 and r[0]["rescales"] == [] and len(r[1]["rescales"]) == 1 and r[1]["start_total"] > _mt(name)[2]
            and whole[0]["rescales"][0][0] == r[0]["L"] + r[1]["rescales"][0][0] and r[1]["rescales"][0][0] % 64 != whole[0]["rescales"][0][0] % 64)


def check_averages():
    """`averages`: an empty bin, integral averages, counts 3 / 7 / 255 / 257, the largest floor(average) a context can hold; and in every
    case with average bytes the double quotient truncates as the exact one does"""
    m = model_run("averages")
    s = np.concatenate([p["sums"] for p in m["parts"]]); n = np.concatenate([p["cnts"] for p in m["parts"]])
    assert (n == 0).any() and {3, 7, 255, 257} <= set(n.ravel().tolist())
    integral = (n > 0) & (s % np.maximum(n, 1) == 0)
    assert integral.sum() >= 4
    bctx = np.concatenate([p["bctx"] for p in m["parts"]])
    assert (bctx == 4 * 128 + 93).any() and (bctx[bctx < 640] % 128).max() == 93
    for name in ("averages", "byte_avg", "byte_avg2", "thr_avg4_equal"):
        m = model_run(name)
        g = build(name)["cfg"]
        for p in m["parts"]:
            if p is None:
                continue
            exact = [(256 * int(a)) // int(b) if b else 0 for a, b in zip(p["sums"].ravel(), p["cnts"].ravel())]
            got = (p["bsym"][0::2] << 8) | p["bsym"][1::2]
            assert got.tolist() == exact, name
    m = model_run("thr_avg4_equal")                               # two equal thresholds: bin 1 never holds a symbol
    assert all((p["cnts"][:, 1] == 0).all() for p in m["parts"])
    return True


def check_lower_bound():
    """n per-base symbols of 1, 63, 64, 65, 4096, 4097; one run holding all of them; every component 0 and every component at its
    largest reachable value present; contexts never coded among the targets"""
    for n in (1, 63, 64, 65, 4096, 4097):
        m = model_run(f"lb_whole_{n}")
        assert [(k[0], r[0]["L"]) for k, r in m["runs"].items()] == [(0, n)], n
        for fam in ("fix2", "avg4"):
            name = f"lb_mixed_{fam}_{n}"
            m, b = model_run(name), build(name)
            g = b["cfg"]
            assert int(b["off"][-1]) == n and len(b["calls"][0]) == (3 if n > 1 else 2)
            tg = all_targets(name)
            absent = [a for f, a in tg if (0, int(model_key(g, a)[0])) not in m["runs"]]
            assert len(absent) >= 2, name
            if n >= 63:
                nf = g["n_fields"]
                assert (0, api_context([0] * nf, 0, 0, 0, 0, 1, 0)) in tg
                assert (0, api_context([g["n_sym"] - 1] * nf, 3, 3, 3, 3, 1, 2 if g["level"] > 1 else 0)) in tg
    return True


def check_bounds():
    """read lengths around every stride; N at 0, 31, 32, len - 1; missing history at every depth; A / AA at the head of an org read;
    each class letter on one (history, bases)"""
    for name in [c["name"] for c in CASES if c["kind"] == "bounds"]:
        b, m = build(name), model_run(name)
        g = b["cfg"]
        lens = set(np.diff(b["off"]).tolist())
        assert set(_BOUND_LENS) <= lens
        api = np.concatenate([p["api"] for p in m["parts"]])
        missing = {sum(1 for t in range(g["n_fields"]) if (a >> (4 * t)) & 0xF == 0xF) for a in api.tolist()} if g["mode"] != ORG else set(range(g["n_fields"] + 1))
        assert missing == set(range(g["n_fields"] + 1))
        for sh in (32, 34, 36, 38):
            assert set(((api >> sh) & 3).tolist()) == {0, 1, 2, 3}
        off, bases = b["off"], b["bases"]
        n_pos = {int(p - off[r]) for r in range(b["n_reads"]) for p in np.flatnonzero(bases[off[r]:off[r + 1]] == 4) + off[r]}
        assert {0, 31, 32} <= n_pos and any(bases[off[r + 1] - 1] == 4 for r in range(b["n_reads"]))
        if g["mode"] == ORG and g["level"] < 3:                   # position 1 after an A: only `i > 1` keeps bm2 == bm1 out
            assert any(bases[off[r]] & 3 == 0 and off[r + 1] - off[r] > 1 for r in range(b["n_reads"]))
        if g["level"] > 1:
            f = b["flags"]
            r0 = b["n_reads"] - 4
            assert [int(f[off[r0 + i]]) for i in range(4)] == list(b"AM P")
            keys = [int(m["parts"][-1]["key"][int(off[r0 + i] - off[part_bounds(b)[-2]]) + 20]) for i in range(4)]
            assert len(set(keys)) == 3 and keys[2] == keys[3]
    return True


def check_parts():
    """1, 63, 64, 65, 129 parts in one call; descending, ascending, equal lengths; empty parts first, in the middle and last; one
    context's run in every part that holds a read"""
    seen = set()
    for c in [c for c in CASES if c["kind"] == "parts"]:
        b, m = build(c["name"]), model_run(c["name"])
        cb = b["calls"][0]
        assert len(b["calls"]) == 1 and len(cb) - 1 == c["n_parts"]
        sizes = [syms_of(b, cb[p], cb[p + 1]) for p in range(c["n_parts"])]
        full = [s for s in sizes if s]
        assert [p for p, s in enumerate(sizes) if not s] == c["empty"]
        k = target_key(c["name"])
        assert all(p is None or (p["key"] == k[1]).any() for p in m["parts"])
        seen.add((c["n_parts"], c["order"], bool(c["empty"])))
        if c["order"] == "desc" and c["n_parts"] > 1:
            assert full[0] > full[-1]
        if c["order"] == "asc":
            assert full[0] < full[-1]
    assert {x[0] for x in seen} == {1, 63, 64, 65, 129} and {x[1] for x in seen} == {"equal", "desc", "asc"} and any(x[2] for x in seen)
    assert BY_NAME["parts_129_desc_empties"]["empty"] == [0, 64, 65, 128] and BY_NAME["parts_65_equal_empties"]["empty"] == [0, 32, 64]
    return True


def check_edges() -> dict:
    """asserts every edge on the cases named for it; returns {edge: [cases]} (DESIGN.md 5d lists the same)"""
    held = {}
    for edge, (names, pred) in EDGES.items():
        for n in names:
            r = _runs(n)
            assert pred(n, r), (edge, n, [(x["call"], x["group"], x["L"], x["start_total"], x["rescales"][:3]) for x in r])
        held[edge] = list(names)
    r = _runs("byte_avg2")                                         # the byte run of one call lies in two parts; the rescale comes in the second
    first_part = int((model_run("byte_avg2")["parts"][0]["bctx"] == 0).sum())
    assert len(r) == 1 and r[0]["rescales"][0][0] > first_part > 0
    assert check_averages()
    held["averages: an empty bin, integral, counts 3 / 7 / 255 / 257, floor 93; double == exact quotient; two equal thresholds"] = ["averages", "byte_avg", "byte_avg2", "thr_avg4_equal"]
    assert check_lower_bound()
    held["lower bound: n = 1, 63, 64, 65, 4096, 4097; a run of the whole input; all-zero and largest contexts; absent contexts"] = [c["name"] for c in CASES if c["kind"].startswith("lb_")]
    assert check_bounds()
    held["read bounds: lengths at every stride, N, missing history, leading A / AA, every class letter"] = [c["name"] for c in CASES if c["kind"] == "bounds"]
    assert check_parts()
    held["parts: 1, 63, 64, 65, 129; descending, ascending, equal; empty first / middle / last"] = [c["name"] for c in CASES if c["kind"] == "parts"]
    held["thresholds: one custom ascending set per bin count, two equal thresholds"] = ["thr_avg2_custom", "thr_fix4_custom", "thr_fix5_custom", "averages", "thr_avg4_equal"]
    for n in held[list(held)[-1]]:
        assert BY_NAME[n].get("fwd") and tuple(BY_NAME[n]["fwd"]) != DEFAULT_T[BY_NAME[n]["mode"]]
    return held


# ---- the case as the reference harness reads it, and the recorded results ----------------------------------------------------
def domain_reads(name: str) -> list:
    """[(first part, end part)] of every model domain: the reference coder, which has no domains, is run once for each"""
    s = domain_starts(name) + [len(part_bounds(build(name))) - 1]
    return list(zip(s, s[1:]))


def case_file(name: str, p0: int | None = None, p1: int | None = None) -> bytes:
    """what oracle/ref_harness/ref_qual.cpp reads: the parts [p0, p1) of the case (default: all)"""
    c, b = BY_NAME[name], build(name)
    g = b["cfg"]
    pb = part_bounds(b)
    p0, p1 = 0 if p0 is None else p0, len(pb) - 1 if p1 is None else p1
    fwd, rev = _thresholds(c)
    out = [b"QUALRUN1", struct.pack("<3I", c["mode"], c.get("source", 0), c["level"]), struct.pack(f"<I{len(fwd)}I", len(fwd), *fwd), struct.pack(f"<I{len(rev)}I", len(rev), *rev)]
    r0, r1 = pb[p0], pb[p1]
    out.append(struct.pack("<I", r1 - r0))
    off = b["off"]
    for r in range(r0, r1):
        s = slice(int(off[r]), int(off[r + 1]))
        out += [struct.pack("<I", s.stop - s.start), b["bases"][s].tobytes(), b["quals"][s].tobytes(), b["flags"][s].tobytes()]
    out.append(struct.pack(f"<I{p1 - p0 + 1}I", p1 - p0, *[x - r0 for x in pb[p0:p1 + 1]]))
    return b"".join(out)


def _thresholds(c):
    return tuple(c.get("fwd") or DEFAULT_T.get(c["mode"], ())), tuple(c.get("rev") or DEFAULT_D.get(c["mode"], ()))


def input_sha(name: str) -> str:
    return hashlib.sha256(case_file(name)).hexdigest()


@functools.lru_cache(maxsize=None)
def golden_cases():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qualruns", "cases.json")
    return {c["name"]: c for c in json.load(open(path))["cases"]}


# ---- the oracle over a case (shared by the CPU and the GPU tests; no part of the model above) -----------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_run(name: str) -> dict:
    """dict(parts = the bytes of every part in order, models = after every call {(family, api context): counters and total},
    decoded = the qualities the oracle's decoder reads back from the parts)"""
    from oracle import pyoracle as O
    c, b = BY_NAME[name], build(name)
    fwd, rev = _thresholds(c)
    new = lambda compress: O.QualCoder(compress, c["mode"], c.get("source", 0), c["level"], fwd, rev)
    starts = set(domain_starts(name))
    qc, dq = new(True), new(False)
    off, parts, models, pi = b["off"], [], [], 0
    decoded = np.zeros(len(b["quals"]), np.uint8)
    fl = b["flags"] if c["level"] > 1 else None
    for cb in b["calls"]:
        for p in range(len(cb) - 1):
            if pi and pi in starts:
                qc, dq = new(True), new(False)
            for r in range(cb[p], cb[p + 1]):
                s = slice(int(off[r]), int(off[r + 1]))
                qc.encode(b["bases"][s], b["quals"][s], None if fl is None else fl[s])
            parts.append(qc.finish_part())
            dq.set_input(parts[-1])
            for r in range(cb[p], cb[p + 1]):
                s = slice(int(off[r]), int(off[r + 1]))
                decoded[s] = dq.decode(b["bases"][s], None if fl is None else fl[s])
            pi += 1
        models.append({t: qc.model(*t) for t in all_targets(name)})
    return dict(parts=parts, models=models, decoded=decoded)


def expected_values(name: str) -> np.ndarray:
    """the qualities (ASCII) a decoder must return, from the input alone (tests/qual_values_ref.py, its integer form)"""
    import qual_values_ref as V
    c, b = BY_NAME[name], build(name)
    fwd, rev = _thresholds(c)
    mode = MODE_NAMES[c["mode"]]
    off = b["off"]
    out = [V.values_int(mode, b["quals"][off[r]:off[r + 1]].astype(np.int64) - 33, list(fwd) or None, list(rev) or None) for r in range(b["n_reads"])]
    return (np.concatenate(out) + 33).astype(np.uint8)
