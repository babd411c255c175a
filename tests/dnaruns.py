"""Constructed tuple streams that put one context run of the DNA coder on every special-cased number of its model kernels
(k_dna_evolve and k_long_find / hist / groups / epochs / apply in csrc/dna.hip) and of its tuple walk.

Three things live here, none of which uses the code under test:
  * a writer of the tuple-stream byte format (csrc/es_format.hpp; utils.h:56-273 of the reference);
  * deterministic, seeded builders of the cases (CASES) at a compression level: reference reads, tuple streams, calls and parts;
  * a small model of what is needed to PROVE that a case sits on its edge: the context recurrences of the constructions
    (plain reads, plain reads with N, read lengths, edit scripts over reference reads) and the adaptive counter model
    (one per symbol at the start, + adder, halve rounding up when the total reaches MAX_TOTAL).
target(case, level) gives the (family, context) run the case aims at, its length in every call, the positions of its rescales
and the final counters; EDGES maps every edge DESIGN.md lists to the cases that hold it, check_edges() asserts each.

What the coders must produce for these streams is not computed here: tests/golden/dnaruns/cases.json records the parts of the
unmodified reference coder (oracle/ref_harness/ref_dna.cpp, tests/golden/make_dnaruns.py)."""
from __future__ import annotations
import functools
import hashlib
import struct
import numpy as np

# ---- the model families, numbered as cl_dna_coder_model / orc_dna_model number them: (symbols, MAX_TOTAL, adder) (dna_coder.h:48-60)
FAMILIES = ("read_type", "rev_comp", "seen", "len_bits", "len_data", "symbols", "symbols_n", "read_id", "read_id_short",
            "anchor_len", "skip_local", "skip_distant", "tuple_type")
FAM = {n: i for i, n in enumerate(FAMILIES)}
_MODEL = {"read_type": (3, 1 << 15, 1), "rev_comp": (2, 1 << 15, 1), "seen": (2, 1 << 15, 1), "len_bits": (32, 1 << 18, 8), "len_data": (256, 1 << 18, 8),
          "symbols": (4, 1 << 10, 1), "symbols_n": (5, 1 << 10, 1), "read_id": (256, 1 << 13, 1), "read_id_short": (None, 1 << 13, 1),
          "anchor_len": (24, 1 << 15, 1), "skip_local": (256, 1 << 15, 1), "skip_distant": (256, 1 << 15, 1), "tuple_type": (8, 1 << 15, 1)}
LEVEL_TS = {1: (2, 5), 2: (3, 7), 3: (4, 8)}          # tuples / symbols of history (dna_coder.cpp:1253-1280)
LEVELS = (1, 3)                                       # the levels the cases are recorded at
DEFAULT_LONG_RUN = 1 << 19                            # dna.hip: LONG_RUN
START_READ_ID = 1000

INS, DEL, MATCH, SUBST, ANCHOR, SKIP, ALT_ID, MAIN_REF, PLAIN, START_PLAIN, START_ES, START_PLAIN_N = range(12)
SUBST_TO_CODE = ((1, 0, 0, 0), (2, 2, 1, 1), (3, 3, 3, 2), (3, 3, 3, 3))     # dna_coder.h:37


def model_params(family: str, max_alt: int):
    n, mt, ad = _MODEL[family]
    return (max_alt if n is None else n), mt, ad


# ---- tuple-stream writer ---------------------------------------------------------------------------------------------
def tuple_bytes(t: int, v1: int = 0, v2: int = 0) -> bytes:
    if t in (INS, SUBST, PLAIN):
        return bytes([(t << 4) | v1])
    if t in (ANCHOR, SKIP):
        assert 0 <= v2 < 1 << 28
        return bytes([(t << 4) | (v2 >> 24), (v2 >> 16) & 255, (v2 >> 8) & 255, v2 & 255])
    if t in (ALT_ID, START_ES):
        return bytes([(t << 4) | v2]) + struct.pack(">I", v1)
    return bytes([t << 4])


def plain_read(bases: np.ndarray, with_n: bool = False):
    """(tuple count, bytes) of a read stored plain: a start tuple and one tuple a base"""
    b = np.asarray(bases, np.uint8)
    return len(b) + 1, bytes([(START_PLAIN_N if with_n else START_PLAIN) << 4]) + ((PLAIN << 4) | b).astype(np.uint8).tobytes()


def script_read(ref_id: int, rev: int, tuples):
    """(tuple count, bytes) of an edit-script read: tuples = [(type, v1, v2), ...] after the start tuple"""
    return len(tuples) + 1, tuple_bytes(START_ES, ref_id, rev) + b"".join(tuple_bytes(*t) for t in tuples)


def parse_tuples(raw: bytes):
    out, p = [], 0
    while p < len(raw):
        t = raw[p] >> 4
        if t in (INS, SUBST, PLAIN):
            out.append((t, raw[p] & 15, 0)); p += 1
        elif t in (ANCHOR, SKIP):
            out.append((t, 0, ((raw[p] & 15) << 24) | (raw[p + 1] << 16) | (raw[p + 2] << 8) | raw[p + 3])); p += 4
        elif t in (ALT_ID, START_ES):
            out.append((t, struct.unpack_from(">I", raw, p + 1)[0], raw[p] & 15)); p += 5
        else:
            out.append((t, 0, 0)); p += 1
    return out


# ---- the adaptive counter model (rc.h:178-185,233-244 of the reference) ------------------------------------------------
def evolve(counts: np.ndarray, syms: np.ndarray, max_total: int, adder: int):
    """Feeds syms to the counters in place.  Returns the rescale positions: p = symbols of syms consumed when a rescale happens
    (1 <= p <= len(syms); p == len(syms): on the last symbol)."""
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
        while int(counts.sum()) >= max_total:
            counts[:] = (counts + 1) // 2
        out.append(pos)


def evolve_one_by_one(counts: np.ndarray, syms, max_total: int, adder: int):
    """The same, a symbol at a time as the reference's model does it: the check of evolve()."""
    out = []
    for i, s in enumerate(syms):
        counts[s] += adder
        if int(counts.sum()) >= max_total:
            while int(counts.sum()) >= max_total:
                counts[:] = (counts + 1) // 2
            out.append(i + 1)
    return out


# ---- context recurrences of the constructions -------------------------------------------------------------------------
def plain_symbols(bases: np.ndarray, S: int):
    """(context, symbol) of every base of a plain read (dna_coder.cpp:1178-1196): the history starts as all ones"""
    b = np.concatenate([np.full(S, 3, np.int64), np.asarray(bases, np.int64)])
    ctx = np.zeros(len(bases), np.int64)
    for t in range(1, S + 1):
        ctx |= b[S - t:S - t + len(bases)] << (2 * (t - 1))
    return ctx << 2, np.asarray(bases, np.int64)


def plain_n_symbols(bases: np.ndarray, S: int):
    """the same for a plain read with Ns (dna_coder.cpp:1213-1227): four bits a symbol, the same mask of 2 S bits"""
    b = np.concatenate([np.full(4, 15, np.int64), np.asarray(bases, np.int64)])
    ctx = np.zeros(len(bases), np.int64)
    for t in range(1, 5):
        ctx |= b[4 - t:4 - t + len(bases)] << (4 * (t - 1))
    return ctx & ((1 << (2 * S)) - 1), np.asarray(bases, np.int64)


def bit_length(x: int) -> int:
    return int(x).bit_length()                                 # ilog2 of basic_coder.h:39-47


def read_len_symbols(length: int):
    """[(family, context, symbol)] of a read length (dna_coder.cpp:1004-1056)"""
    nb = bit_length(length)
    out = [("len_bits", 0, nb)]
    if nb < 2:
        return out
    ctx = nb << 3
    length -= 1 << (nb - 1)
    if nb <= 9:
        return out + [("len_data", ctx, length)]
    prefix = length >> (nb - 9)
    suffix = length - (prefix << (nb - 9))
    out.append(("len_data", ctx, prefix))
    nb -= 9; ctx += 4
    while nb > 0:
        out.append(("len_data", ctx, suffix & 255)); suffix >>= 8; ctx += 1; nb -= 8
    return out


def script_symbols(raw: bytes, refs, level: int, stats: dict | None = None):
    """[(family, context, symbol)] of the tuple-type, anchor-length, orientation, seen and short-id symbols of one edit-script read
    (CDNACoder::Encode, dna_coder.cpp:65-231,489-509,572-615,651-710,958-978) in coding order.  Asserts that every reference symbol
    read is a base: the constructions stay inside their reference reads."""
    T, S = LEVEL_TS[level]
    mask_t, mask_s = (1 << (3 * T)) - 1, (1 << (2 * S)) - 1
    tup = parse_tuples(raw)
    assert tup[0][0] == START_ES
    out = []
    ctx_tuple, ctx_symbol, ctx_rev = mask_t, mask_s, 0xf
    cached = set()

    def rev_comp(rid, rc):
        nonlocal ctx_rev
        if rid in cached:
            return
        out.append(("rev_comp", ctx_rev, rc)); cached.add(rid)
        ctx_rev = ((ctx_rev << 2) + rc) & 0xf

    def oriented(rid, rc):
        r = np.asarray(refs[rid], np.int64)
        return (3 - r[::-1]) if rc else r

    ref = oriented(tup[0][1], tup[0][2])
    rev_comp(tup[0][1], tup[0][2])
    alt_ids, alt_pos_of, alt_read = {}, {}, {}
    alt, alt_id = None, -1
    ref_pos = alt_pos = delta = 0
    is_main, first, last_flag = True, True, None
    for t, v1, v2 in tup[1:]:
        cur, pos = (ref, ref_pos) if is_main else (alt, alt_pos)
        assert 0 <= pos < len(cur), "a reference position past the end of its read"
        ref_symbol = int(cur[pos])
        shift = 3 * T
        ctx = ctx_tuple + ((ctx_symbol & 0xf) << shift) + (ref_symbol << (shift + 4))
        ctx += (1 if delta < -10 else 2 if delta < -1 else 3 if delta > 10 else 4 if delta > 1 else 0) << (shift + 6)
        if not first:
            assert t not in {MATCH: (ANCHOR,), DEL: (SKIP,), ANCHOR: (ANCHOR, MATCH), SKIP: (DEL, SKIP), MAIN_REF: (ALT_ID, MAIN_REF), ALT_ID: (ALT_ID, MAIN_REF)}.get(last_flag, ()), "an excluded tuple type"
        out.append(("tuple_type", ctx, t))
        ctx_tuple = ((ctx_tuple << 3) + t) & mask_t
        first, last_flag = False, t
        if t == ALT_ID:
            if not is_main:
                alt_pos_of[alt_id] = alt_pos
            if not alt_ids:
                alt_ids[v1] = 0; new = True
            else:
                seen = len(alt_ids)
                new = v1 not in alt_ids
                out.append(("seen", seen, 0 if new else 1))
                if new:
                    alt_ids[v1] = seen
                else:
                    out.append(("read_id_short", seen, alt_ids[v1]))
            if new:
                alt_read[v1] = oriented(v1, v2); alt_pos_of.setdefault(v1, 0)
            rev_comp(v1, v2)
            alt_id, alt, alt_pos, is_main, delta = v1, alt_read[v1], 0, False, 0
        elif t == ANCHOR:
            length, part = v2, 0
            while length:
                if length < 23:
                    out.append(("anchor_len", part, length)); break
                out.append(("anchor_len", part, 23)); length -= 22; part += 1
            if is_main:
                ref_pos += v2
            else:
                alt_pos += v2
            cur, pos = (ref, ref_pos) if is_main else (alt, alt_pos)
            assert pos - S >= 0 and pos <= len(cur), "an anchor whose history leaves the reference read"
            for i in range(S, 0, -1):
                ctx_symbol = (ctx_symbol << 2) + int(cur[pos - i])
            ctx_symbol &= mask_s
            delta = 0
        elif t == MATCH:
            ctx_symbol = ((ctx_symbol << 2) + ref_symbol) & mask_s
            if is_main: ref_pos += 1
            else: alt_pos += 1
        elif t == INS:
            ctx_symbol = ((ctx_symbol << 2) + v1) & mask_s
            delta += 1
        elif t == DEL:
            if is_main: ref_pos += 1
            else: alt_pos += 1
            delta -= 1
        elif t == SUBST:
            assert v1 < 3
            ctx_symbol = ((ctx_symbol << 2) + SUBST_TO_CODE[v1][ref_symbol]) & mask_s
            if is_main: ref_pos += 1
            else: alt_pos += 1
        elif t == SKIP:
            delta -= v2
            if is_main: ref_pos += v2
            else: alt_pos += v2
        elif t == MAIN_REF:
            is_main = True
            alt_pos_of[alt_id] = alt_pos
            delta = 0
        else:
            raise AssertionError(f"tuple type {t} inside a script")
    if stats is not None:
        stats["cached_ids"] = stats.get("cached_ids", []) + [len(cached)]
        stats["n_alt"] = stats.get("n_alt", []) + [len(alt_ids)]
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------
# Every case: kind (its builder), seed, long_run (the COLORD_HIP_LONG_RUN of the long-path pass), and per kind:
#   plain / plain_n   calls = [[L of part 0, L of part 1, ...], ...]: one read a part with exactly L symbols in the target context
#                     (the context "all of the history is T" / "all of the history is zero"); L = ("rescale", ...): the position of a
#                     rescale of the run that Lmax symbols would make (_rescale_pos)
#   lengths           calls = [[reads of part 0, ...], ...]: tiny plain reads, lengths 4..7 (with a few of 1..3)
#   anchor_x          calls = [[pairs of part 0, ...], ...]: reads of ANCHOR X ANCHOR X ... over a homopolymer, X in {DEL, SUBST, INS, SKIP}
#   match_x           the same with reads of M^T X M^T X ... after one long SKIP
#   alts              max_alt; reads that use max_alt alternative references, revisit them and return to the one cached last
CASES = [
    dict(name="sym_below_long_run", kind="plain", seed=11, long_run=4096, calls=[[4095]]),
    dict(name="sym_at_long_run", kind="plain", seed=12, long_run=4096, calls=[[4096]]),
    dict(name="sym_above_long_run", kind="plain", seed=13, long_run=4096, calls=[[4097]]),
    dict(name="sym_no_rescale_then_one_short", kind="plain", seed=14, long_run=1000, calls=[[1019], [1100]]),
    dict(name="sym_rescale_on_last", kind="plain", seed=15, long_run=4096, calls=[[("rescale", 9, 8000)]]),
    dict(name="sym_rescale_on_last_step_bound", kind="plain", seed=18, long_run=4096, calls=[[("rescale_mod", 64, 4096, 60000)]]),
    dict(name="sym_rescale_on_last_group_bound", kind="plain", seed=None, long_run=4096, calls=[[("rescale_mod", 4096, 0, 300000)]]),
    dict(name="sym_two_parts", kind="plain", seed=16, long_run=4096, calls=[[3000, 3000]]),
    dict(name="sym_two_calls", kind="plain", seed=17, long_run=4096, calls=[[5000], [5000]]),
    dict(name="sym_giant_then_symn", kind="plain", seed=None, long_run=4096, calls=[[300000]], second=dict(kind="plain_n", L=5000)),
    dict(name="symn_long", kind="plain_n", seed=21, long_run=4096, calls=[[4160]]),
    dict(name="lengths_at_long_run", kind="lengths", seed=30, long_run=4096, calls=[[4096]]),
    dict(name="lengths_rescale_on_last", kind="lengths", seed=31, long_run=4096, calls=[[32764]]),
    dict(name="lengths_two_rescales", kind="lengths", seed=32, long_run=4096, calls=[[40000, 30000]]),
    dict(name="anchor_x", kind="anchor_x", seed=41, long_run=4096, calls=[[20000, 20000]]),
    dict(name="anchor_x_two_calls", kind="anchor_x", seed=42, long_run=4096, calls=[[30000], [6000]]),
    dict(name="match_x", kind="match_x", seed=51, long_run=4096, calls=[[36000]]),
    dict(name="alts_1", kind="alts", seed=61, long_run=64, max_alt=1, walk_chunk=32, calls=[[3]]),
    dict(name="alts_32", kind="alts", seed=62, long_run=64, max_alt=32, walk_chunk=32, calls=[[2]]),
    dict(name="alts_33", kind="alts", seed=63, long_run=64, max_alt=33, walk_chunk=32, calls=[[2]]),
    dict(name="alts_64", kind="alts", seed=64, long_run=64, max_alt=64, walk_chunk=32, calls=[[2, 1]]),
]
GIANT_SEEDS = {1: 1011, 3: 1011}                      # seeds with a rescale on a multiple of 4096, found by find_giant_seed()
BY_NAME = {c["name"]: c for c in CASES}
MIX = np.array([0.20, 0.15, 0.10, 0.55])               # A C G T among the symbols of the target context of the plain cases
MIX_N = np.array([0.50, 0.15, 0.15, 0.10, 0.10])       # A C G T N


def _plain_target_read(rng, L: int, S: int):
    """a read with exactly L positions whose S previous bases are all T: the chosen symbols, S filler Ts after every one that is no T"""
    q = rng.choice(4, size=L, p=MIX)
    rep = np.where(q == 3, 1, S + 1)
    out = np.full(int(rep.sum()), 3, np.uint8)
    out[np.cumsum(rep) - rep] = q
    if q[-1] != 3:
        out = out[:len(out) - S]                          # (nothing after the last symbol)
    return out, q


def _plain_n_target_read(rng, L: int, S: int):
    """a read with exactly L positions whose history is all zero: four zeros first, and after every symbol that is not zero; cut after the
    L-th such position (where the mask keeps fewer than four symbols, filler zeros are in that context too)"""
    q = rng.choice(5, size=L, p=MIX_N)
    rep = np.where(q == 0, 1, 5)
    out = np.zeros(4 + int(rep.sum()), np.uint8)
    out[4 + np.cumsum(rep) - rep] = q
    ctx, sym = plain_n_symbols(out, S)
    out = out[:np.flatnonzero(ctx == 0)[L - 1] + 1]
    return out, sym[:len(out)][ctx[:len(out)] == 0]


def _rescale_pos(kind, seed, S, spec):
    """L = the position of a rescale of the run that spec[-1] symbols would make: ("rescale", k, Lmax) the k-th;
    ("rescale_mod", m, not_m, Lmax) the first at or above 4096 on a multiple of m and (not_m > 0) of no multiple of not_m"""
    rng = np.random.default_rng(seed)
    q = (_plain_target_read(rng, spec[-1], S) if kind == "plain" else _plain_n_target_read(rng, spec[-1], S))[1]
    n, mt, ad = _MODEL["symbols" if kind == "plain" else "symbols_n"]
    pos = evolve(np.ones(n, np.int64), q, mt, ad)
    if spec[0] == "rescale":
        return pos[spec[1]]
    return next(p for p in pos if p >= 4096 and p % spec[1] == 0 and (not spec[2] or p % spec[2]))


def _homopolymer_reads(rng, kind, n_units, T):
    """reads of at most 400 units over reference read 0 (all A, 20 k long): [(tuple count, bytes)]"""
    reads, left = [], n_units
    while left:
        n = min(left, 400); left -= n
        tup = []
        if kind == "match_x":
            tup.append((SKIP, 0, 1000))                                # delta stays far below -10: one delta class for the whole read
        for u in range(n):
            if kind == "anchor_x":
                # (the first anchor reaches past the S symbols of history it loads; lengths of 23 and more take a second symbol, in context 1)
                tup.append((ANCHOR, 0, int(rng.integers(8 if u == 0 else 1, 31))))
                x = int(rng.choice([DEL, SUBST, INS, SKIP], p=[0.5, 0.2, 0.2, 0.1]))
            else:
                tup += [(MATCH, 0, 0)] * (T + int(rng.integers(0, 2)))
                x = int(rng.choice([DEL, SUBST, INS, SKIP], p=[0.3, 0.3, 0.25, 0.15]))
            if x == SKIP:
                tup.append((SKIP, 0, int(rng.integers(10, 20))))
            elif x == DEL:
                tup.append((DEL, 0, 0))
            else:
                tup.append((x, int(rng.integers(0, 3 if x == SUBST else 4)), 0))
        reads.append(script_read(0, 0, tup))
    return reads


def _alt_read(rng, n_alt, lens, back_to_last=True):
    """one read over main reference 0 and alternatives 1..n_alt (reference ids): every alternative once, then again in another order, then the
    one used (and cached) last: units ALT_ID SKIP ANCHOR, so that chunks of 32 tuples begin on each of the three"""
    order = [int(x) for x in 1 + rng.permutation(n_alt)]
    again = [int(x) for x in 1 + rng.permutation(n_alt)]
    if again[0] == order[-1] and n_alt > 1:
        again = again[1:] + again[:1]
    visits = order + again + ([order[-1]] if back_to_last and again[-1] != order[-1] else [])
    revs = {i: int(rng.integers(0, 2)) for i in range(1, n_alt + 1)}
    tup, left_at = [(ANCHOR, 0, 20)], {}
    prev = None
    for rid in visits:
        if rid == prev:                                                    # (an alternative cannot follow itself directly: go through the main reference)
            tup += [(MAIN_REF, 0, 0), (MATCH, 0, 0)]
        s = int(rng.integers(1, 40))
        a = int(rng.integers(9, 30))
        tup += [(ALT_ID, rid, revs[rid]), (SKIP, 0, s), (ANCHOR, 0, a)]
        assert s + a < lens[rid]
        left_at[rid] = s + a
        prev = rid
    tup += [(MAIN_REF, 0, 0), (MATCH, 0, 0), (SUBST, 1, 0), (MATCH, 0, 0)]
    return script_read(0, int(rng.integers(0, 2)), tup), visits


@functools.lru_cache(maxsize=None)
def build(name: str, level: int):
    """dict(refs, reads=[(tuple count, bytes)], calls=[read bounds of the parts of call 0, ...] (global read numbers), max_alt, runs)"""
    c = BY_NAME[name]
    T, S = LEVEL_TS[level]
    seed = c["seed"] if c["seed"] is not None else GIANT_SEEDS[level]
    rng = np.random.default_rng(seed)
    refs, reads, calls = [np.array([0, 1, 2, 3] * 4, np.uint8)], [], []
    kind = c["kind"]
    if kind in ("anchor_x", "match_x"):
        refs = [np.zeros(20000, np.uint8)]
    if kind == "alts":
        lens = [400] + [int(x) for x in rng.integers(80, 120, size=c["max_alt"])]
        refs = [rng.integers(0, 4, size=n).astype(np.uint8) for n in lens]
    visits = []
    for parts in c["calls"]:
        bounds = [len(reads)]
        for L in parts:
            if isinstance(L, tuple):
                L = _rescale_pos(kind, seed, S, L)
            if kind == "plain":
                reads.append(plain_read(_plain_target_read(rng, L, S)[0]))
            elif kind == "plain_n":
                reads.append(plain_read(_plain_n_target_read(rng, L, S)[0], True))
            elif kind == "lengths":
                lens_ = np.where(rng.random(L) < 0.9, rng.integers(4, 8, size=L), rng.integers(1, 4, size=L))
                for n in lens_:
                    reads.append(plain_read(rng.integers(0, 4, size=int(n))))
            elif kind in ("anchor_x", "match_x"):
                reads += _homopolymer_reads(rng, kind, L, T)
            elif kind == "alts":
                for _ in range(L):
                    r, v = _alt_read(rng, c["max_alt"], lens)
                    reads.append(r); visits.append(v)
            bounds.append(len(reads))
        if "second" in c and len(calls) + 1 == len(c["calls"]):
            reads.append(plain_read(_plain_n_target_read(rng, c["second"]["L"], S)[0], True))
            bounds[-1] = len(reads)
        calls.append(bounds)
    return dict(refs=refs, reads=reads, calls=calls, max_alt=c.get("max_alt", 5), visits=visits)


def case_file(name: str, level: int) -> bytes:
    """the case as oracle/ref_harness/ref_dna.cpp reads it; its SHA-256 is the input hash of cases.json"""
    b = build(name, level)
    out = [b"DNARUNS1", struct.pack("<III", level, b["max_alt"], START_READ_ID), struct.pack("<I", len(b["refs"]))]
    for r in b["refs"]:
        out += [struct.pack("<I", len(r)), np.asarray(r, np.uint8).tobytes()]
    out.append(struct.pack("<I", len(b["reads"])))
    for nt, raw in b["reads"]:
        out += [struct.pack("<II", nt, len(raw)), raw]
    bounds = [0] + [x for cb in b["calls"] for x in cb[1:]]
    out.append(struct.pack("<I", len(bounds) - 1) + struct.pack(f"<{len(bounds)}I", *bounds))
    return b"".join(out)


def input_sha(name: str, level: int) -> str:
    return hashlib.sha256(case_file(name, level)).hexdigest()


_SCRIPT_CACHE = {}


def read_target_symbols(name: str, level: int, i: int, fam: str, ctx: int, stats=None) -> np.ndarray:
    """the symbols read i of a built case codes in model (fam, ctx), in coding order (read_type is left to target(): it chains over reads)"""
    T, S = LEVEL_TS[level]
    b = build(name, level)
    nt, raw = b["reads"][i]
    t0 = raw[0] >> 4
    if fam in ("len_bits", "len_data"):
        return np.array([s for f, x, s in read_len_symbols(nt - 1) if f == fam and x == ctx], np.int64)
    if fam == "symbols" and t0 == START_PLAIN:
        c, sym = plain_symbols(np.frombuffer(raw, np.uint8)[1:] & 15, S)
        return sym[c == ctx]
    if fam == "symbols_n" and t0 == START_PLAIN_N:
        c, sym = plain_n_symbols(np.frombuffer(raw, np.uint8)[1:] & 15, S)
        return sym[c == ctx]
    if t0 == START_ES and fam in ("tuple_type", "anchor_len", "rev_comp", "seen", "read_id_short"):
        key = (name, level, i)
        if key not in _SCRIPT_CACHE:
            st = {}
            _SCRIPT_CACHE[key] = (script_symbols(raw, b["refs"], level, st), st)
        syms, st = _SCRIPT_CACHE[key]
        if stats is not None:
            for k, v in st.items():
                stats[k] = stats.get(k, []) + v
        return np.array([s for f, x, s in syms if f == fam and x == ctx], np.int64)
    return np.zeros(0, np.int64)


def _target_of(c, level):
    """(family, context) of the run a case aims at, and of the second run of the case that has one"""
    T, S = LEVEL_TS[level]
    kind = c["kind"]
    if kind == "plain":
        t = ("symbols", ((1 << (2 * S)) - 1) << 2)
    elif kind == "plain_n":
        t = ("symbols_n", 0)
    elif kind == "lengths":
        t = ("len_bits", 0)
    elif kind == "anchor_x":
        t = ("anchor_len", 0)
    elif kind == "match_x":
        # after T matches over A, far behind the reference (delta < -10): the last T tuple types are matches, the last two symbols and the reference symbol are A
        t = ("tuple_type", sum(MATCH << (3 * i) for i in range(T)) + (1 << (3 * T + 6)))
    else:
        t = ("read_id_short", c["max_alt"])
    return t


def extra_targets(c, level):
    """further (family, context) runs of a case that the tests compare as well"""
    T, S = LEVEL_TS[level]
    if "second" in c:
        return [("symbols_n", 0)]
    if c["kind"] == "lengths":
        return [("len_data", 3 << 3), ("read_type", 0)]
    if c["kind"] == "anchor_x":
        # X after an anchor, itself after a deletion (level 3: and an anchor and a deletion before): the two-exclusion form; history and reference symbol A, delta 0
        hist = [DEL, ANCHOR] * (T // 2)
        return [("tuple_type", sum(t << (3 * (T - 1 - i)) for i, t in enumerate(hist)))]
    if c["kind"] == "alts":
        return [("seen", c["max_alt"]), ("rev_comp", 0)]
    return []


@functools.lru_cache(maxsize=None)
def target(name: str, level: int, which: int = 0):
    """The run a case aims at (which = 0) or one of its further runs: dict(family, context, n_sym, max_total, adder, L = [symbols in call 0, ...],
    rescales = [[positions within call 0's run], ...], start_total = [the model's total when call i starts], counts = final counters, total)."""
    c, b = BY_NAME[name], build(name, level)
    fam, ctx = ([_target_of(c, level)] + extra_targets(c, level))[which]
    n, mt, ad = model_params(fam, b["max_alt"])
    counts = np.ones(n, np.int64)
    Ls, rescales, starts, stats, rt_ctx = [], [], [], {}, 0
    for cb in b["calls"]:
        if fam == "read_type":                                             # the types of the four reads before, also across calls (dna_coder.cpp:440-463)
            syms = []
            for i in range(cb[0], cb[-1]):
                flag = {START_PLAIN: 0, START_PLAIN_N: 1}.get(b["reads"][i][1][0] >> 4, 2)
                if rt_ctx == ctx:
                    syms.append(flag)
                rt_ctx = ((rt_ctx << 2) + flag) & 0xff
            syms = np.array(syms, np.int64)
        else:
            syms = np.concatenate([read_target_symbols(name, level, i, fam, ctx, stats) for i in range(cb[0], cb[-1])] + [np.zeros(0, np.int64)])
        starts.append(int(counts.sum()))
        Ls.append(len(syms))
        rescales.append(evolve(counts, syms, mt, ad))
    return dict(family=fam, context=ctx, n_sym=n, max_total=mt, adder=ad, L=Ls, rescales=rescales, start_total=starts,
                counts=counts.copy(), total=int(counts.sum()), stats=stats)


def find_giant_seed(level: int, start: int = 1000) -> int:
    """the first seed from `start` whose giant run has a rescale on a multiple of 4096 (how GIANT_SEEDS was filled)"""
    T, S = LEVEL_TS[level]
    L = BY_NAME["sym_giant_then_symn"]["calls"][0][0]
    n, mt, ad = _MODEL["symbols"]
    for seed in range(start, start + 1000):
        q = _plain_target_read(np.random.default_rng(seed), L, S)[1]
        if any(p % 4096 == 0 for p in evolve(np.ones(n, np.int64), q, mt, ad)):
            return seed
    raise AssertionError("no seed found")


# ---- the edges and the cases that hold them ------------------------------------------------------------------------------
def _runs(name, level, which=0):
    t = target(name, level, which)
    return t, list(zip(t["L"], t["rescales"], t["start_total"]))


def _class(t):
    return 8 if t["n_sym"] <= 8 else 32 if t["n_sym"] <= 32 else 256


EDGES = {
    # name: (cases, predicate over (case dict, target, [(L, rescales, total at start) of each call]))
    "L == long_run - 1": (["sym_below_long_run"], lambda c, t, r: r[0][0] == c["long_run"] - 1),
    "L == long_run": (["sym_at_long_run", "lengths_at_long_run"], lambda c, t, r: r[0][0] == c["long_run"]),
    "L == long_run + 1": (["sym_above_long_run"], lambda c, t, r: r[0][0] == c["long_run"] + 1),
    "L % 64 == 0": (["sym_at_long_run", "symn_long"], lambda c, t, r: r[0][0] % 64 == 0 and r[0][0] >= c["long_run"]),
    "L % 64 == 1": (["sym_above_long_run"], lambda c, t, r: r[0][0] % 64 == 1 and r[0][0] >= c["long_run"]),
    "L % 64 == 63": (["sym_below_long_run"], lambda c, t, r: r[0][0] % 64 == 63),
    "L % 4096 == 0": (["sym_at_long_run"], lambda c, t, r: r[0][0] % 4096 == 0 and r[0][0] >= c["long_run"]),
    "L % 4096 == 1": (["sym_above_long_run"], lambda c, t, r: r[0][0] % 4096 == 1 and r[0][0] >= c["long_run"]),
    "L > 262144 (a second sweep of k_long_groups)": (["sym_giant_then_symn"], lambda c, t, r: r[0][0] > 262144),
    "a run with no rescale": (["sym_no_rescale_then_one_short"], lambda c, t, r: r[0][1] == [] and r[0][0] >= c["long_run"]),
    "a rescale at p == L": (["sym_rescale_on_last", "lengths_rescale_on_last"], lambda c, t, r: r[0][1][-1] == r[0][0] and r[0][0] >= c["long_run"]),
    "a rescale at p == L, L % 64 == 0": (["sym_rescale_on_last_step_bound"], lambda c, t, r: r[0][1][-1] == r[0][0] and r[0][0] % 64 == 0 and r[0][0] % 4096 and r[0][0] >= c["long_run"]),
    "a rescale at p == L, L % 4096 == 0": (["sym_rescale_on_last_group_bound"], lambda c, t, r: r[0][1][-1] == r[0][0] and r[0][0] % 4096 == 0 and r[0][0] >= c["long_run"]),
    "a rescale at p % 64 == 0": (["sym_giant_then_symn"], lambda c, t, r: any(p % 64 == 0 and p % 4096 for p in r[0][1])),
    "a rescale at p % 4096 == 0": (["sym_giant_then_symn"], lambda c, t, r: any(p % 4096 == 0 for p in r[0][1])),
    "a rescale in mid-step": (["sym_above_long_run", "anchor_x"], lambda c, t, r: any(p % 64 for p in r[0][1])),
    "a call that starts one symbol below MAX_TOTAL": (["sym_no_rescale_then_one_short"], lambda c, t, r: r[1][2] == t["max_total"] - t["adder"] and r[1][1][0] == 1 and r[1][0] >= c["long_run"]),
    "a run split across two parts": (["sym_two_parts", "anchor_x", "lengths_two_rescales"], lambda c, t, r: len(c["calls"][0]) == 2 and r[0][0] >= c["long_run"] and
                                     (c["kind"] != "plain" or max(c["calls"][0]) < c["long_run"])),
    "a run split across two calls": (["sym_two_calls", "anchor_x_two_calls"], lambda c, t, r: len(r) == 2 and min(x[0] for x in r) >= c["long_run"] and t["start_total"][1] > t["n_sym"]),
    "a 32-class run: len_bits": (["lengths_two_rescales"], lambda c, t, r: t["family"] == "len_bits" and _class(t) == 32 and len(r[0][1]) >= 2 and r[0][0] >= c["long_run"]),
    "a 32-class run: anchor_len": (["anchor_x", "anchor_x_two_calls"], lambda c, t, r: t["family"] == "anchor_len" and _class(t) == 32 and sum(len(x[1]) for x in r) >= 1 and r[0][0] >= c["long_run"]),
    "an 8-class run with one exclusion": (["match_x"], lambda c, t, r: t["family"] == "tuple_type" and len(r[0][1]) >= 1 and r[0][0] >= c["long_run"]),
}
# edges of a case's further runs: (case, which, predicate)
EDGES_EXTRA = {
    "a second long run after a giant one, in the same group": ("sym_giant_then_symn", 1, lambda c, t, r: t["family"] == "symbols_n" and r[0][0] >= c["long_run"] and len(r[0][1]) >= 1),
    "a run of more than 32 symbols' family (len_data) longer than long_run": ("lengths_two_rescales", 1, lambda c, t, r: _class(t) == 256 and r[0][0] >= c["long_run"] and len(r[0][1]) >= 1),
    "an 8-class run with two exclusions": ("anchor_x", 1, lambda c, t, r: t["family"] == "tuple_type" and r[0][0] >= c["long_run"]),
}


def check_alts(name: str, level: int):
    """the alternative-reference cases: every read uses max_alt alternatives, comes back to each, and ends on the id cached last (the
    (max_alt + 1)-th id of the orientation cache, after the main reference); chunks of 32 tuples begin on an alt-id tuple, on the skip
    after one and on an anchor"""
    c, b = BY_NAME[name], build(name, level)
    t = target(name, level)
    n_reads = len(b["reads"])
    assert t["stats"]["n_alt"] == [c["max_alt"]] * n_reads and t["stats"]["cached_ids"] == [c["max_alt"] + 1] * n_reads
    firsts = set()
    for (nt, raw), visits in zip(b["reads"], b["visits"]):
        order = list(dict.fromkeys(visits))
        assert len(order) == c["max_alt"] and visits[-1] == order[-1] and visits.count(order[-1]) >= 2
        tup = parse_tuples(raw)[1:]
        for k in range(c["walk_chunk"], len(tup), c["walk_chunk"]):
            firsts.add("skip after alt-id" if tup[k][0] == SKIP and tup[k - 1][0] == ALT_ID else {ALT_ID: "alt-id", ANCHOR: "anchor"}.get(tup[k][0], "other"))
    if c["max_alt"] >= 32:
        assert {"alt-id", "skip after alt-id", "anchor"} <= firsts, firsts
    assert t["L"][0] >= 1                                                 # short ids coded with every alternative seen
    return firsts


def check_edges(level: int):
    """asserts every edge on the cases named for it; returns {edge: [cases]} (DESIGN.md 5c lists the same)"""
    held = {}
    for edge, (names, pred) in EDGES.items():
        for n in names:
            t, r = _runs(n, level)
            assert pred(BY_NAME[n], t, r), (edge, n, level, t["L"], [x[:5] for x in t["rescales"]])
        held[edge] = names
    for edge, (n, which, pred) in EDGES_EXTRA.items():
        t, r = _runs(n, level, which)
        assert pred(BY_NAME[n], t, r), (edge, n, level, t["family"], t["L"], [x[:5] for x in t["rescales"]])
        held[edge] = [n]
    for n in ("alts_1", "alts_32", "alts_33", "alts_64"):
        check_alts(n, level)
    held["max_alt_refs 1, 32, 33, 64; all used, revisited, back to the id cached last; chunk bounds on alt-id, skip, anchor"] = ["alts_1", "alts_32", "alts_33", "alts_64"]
    return held


# ---- the oracle over a case (shared by the CPU and the GPU tests; no part of the model above) -----------------------------------------------
def all_targets(name: str, level: int):
    c = BY_NAME[name]
    return [_target_of(c, level)] + extra_targets(c, level)


@functools.lru_cache(maxsize=None)
def golden_cases():
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dnaruns", "cases.json")
    return {c["name"]: c for c in json.load(open(path))["cases"]}


@functools.lru_cache(maxsize=None)
def oracle_run(name: str, level: int):
    """dict(parts = the bytes of every part in order, models = after every call {(family, context): counters and total})"""
    from oracle import pyoracle as O
    b = build(name, level)
    dc = O.DnaCoder(b["max_alt"], level, START_READ_ID)
    for r in b["refs"]:
        dc.add_ref(r)
    parts, models = [], []
    for cb in b["calls"]:
        for p in range(len(cb) - 1):
            for i in range(cb[p], cb[p + 1]):
                dc.encode(b["reads"][i][1], b["reads"][i][0])
            parts.append(dc.finish_part())
        models.append({(f, x): dc.model(FAM[f], x) for f, x in all_targets(name, level)})
    return dict(parts=parts, models=models)
