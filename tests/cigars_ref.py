"""The base-level CIGAR of every overlap record in plain Python, written from the definition over the byte format: a visit's tuples
become a list of (operation, length) pairs, the list is cut at its first and last aligned pair, and equal neighbours are summed by groupby.  Nothing
here keeps an open run or a count of kept runs in a loop the way the kernel and the host twin do.  The visits, the format and the validity checks
(with their texts) are those of tests/overlaps_ref.py and tests/edits_ref.py."""
import struct
from itertools import groupby
import numpy as np
import overlaps_ref as OR
from edits_ref import INS, DEL, MATCH, SUBST, ANCHOR, SKIP, START_ES

OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8                        # BAM's codes
CHAR = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
OP_OF = {INS: OP_I, DEL: OP_D, MATCH: OP_EQ, SUBST: OP_X, ANCHOR: OP_EQ, SKIP: OP_D}
RUN_LIMIT = 1 << 28                                         # a merged run of this many bases or more does not fit 28 bits
VERSION, OP_BYTES, HEAD = 1, 4, 24
RUN_TEXT = "a CIGAR operation of 2^28 bases or more"


class TooLong(Exception):
    def __init__(self, read):
        super().__init__(f"read {read}: {RUN_TEXT}")
        self.read = read


def cigar_of_visit(tuples):
    """[(op, len)] of a visit's tuples [(type, value)], or None for a visit without an aligned column"""
    pairs = [(OP_OF[t], 1 if t <= SUBST else v) for t, v in tuples]
    pairs = [(op, n) for op, n in pairs if n > 0]
    aligned = [i for i, (op, _) in enumerate(pairs) if op in (OP_EQ, OP_X)]
    if not aligned:
        return None
    return [(op, sum(n for _, n in grp)) for op, grp in groupby(pairs[aligned[0]:aligned[-1] + 1], key=lambda p: p[0])]


def cigars_of_read(stream, refs, id_limit=0, read=0):
    """the CIGARs of a read's records, one [(op, len)] per record of overlaps_ref in its order; [] for a record on a reference id at or past id_limit
    (0: every reference).  Raises Malformed as overlaps_ref does, then TooLong."""
    stream = bytes(stream)
    OR.records_of_read(stream, refs, read=read)              # every check of the walk, with its text
    if stream[0] >> 4 != START_ES:
        return []
    out = []
    for rid, _, _, tuples in OR.visits_of(stream):
        cg = cigar_of_visit(tuples)
        if cg is not None:
            out.append(cg if not id_limit or rid < id_limit else [])
    if any(n >= RUN_LIMIT for cg in out for _, n in cg):
        raise TooLong(read)
    return out


def words(cg):
    return [(n << 4) | op for op, n in cg]


def cigars(streams, refs, id_limit=0):
    """(the operation count of every record, the operations len << 4 | op one record behind the other), two uint32 arrays"""
    per = [cg for r, s in enumerate(streams) for cg in cigars_of_read(s, refs, id_limit, r)]
    return np.array([len(cg) for cg in per], np.uint32), np.array([w for cg in per for w in words(cg)], np.uint32)


def split(rec_ops, ops):
    """the operations of every record as a list of (op, len)"""
    off = np.concatenate([[0], np.cumsum(np.asarray(rec_ops, np.uint64))]).astype(np.int64)
    return [[(int(w) & 0xf, int(w) >> 4) for w in ops[off[i]:off[i + 1]]] for i in range(len(rec_ops))]


def invariants(recs, rec_ops, ops, zero_ok=False):
    """the relations between every record (n, 12) and its operations; returns what is broken as (record index, name).  zero_ok: a record with the
    count 0 (id_limit) is skipped."""
    bad = []
    recs = np.asarray(recs, np.uint32).reshape(-1, 12)
    if len(recs) != len(rec_ops) or int(np.asarray(rec_ops, np.uint64).sum()) != len(ops):
        return [(-1, "counts")]
    for i, (rec, cg) in enumerate(zip(recs, split(rec_ops, ops))):
        if zero_ok and not cg:
            continue
        d = dict(zip(OR.FIELDS, (int(x) for x in rec)))
        total = lambda which: sum(n for op, n in cg if op in which)
        checks = {"query": total((OP_EQ, OP_X, OP_I)) == d["qe"] - d["qs"], "target": total((OP_EQ, OP_X, OP_D)) == d["te"] - d["ts"], "matches": total((OP_EQ,)) == d["matches"],
                  "subst": total((OP_X,)) == d["subst"], "ends": bool(cg) and cg[0][0] in (OP_EQ, OP_X) and cg[-1][0] in (OP_EQ, OP_X),
                  "merged": all(a[0] != b[0] for a, b in zip(cg, cg[1:])), "lengths": all(n >= 1 for _, n in cg), "codes": all(op in CHAR for op, _ in cg)}
        bad += [(i, k) for k, ok in checks.items() if not ok]
    return bad


def pack_hipcigars(rec_ops, ops, version=VERSION, op_bytes=OP_BYTES, records=None, operations=None):
    rec_ops, ops = np.asarray(rec_ops, "<u4"), np.asarray(ops, "<u4")
    return struct.pack("<IIQQ", version, op_bytes, len(rec_ops) if records is None else records, len(ops) if operations is None else operations) + rec_ops.tobytes() + ops.tobytes()


def text(cg, rev=False):
    """CIGAR text, the target forward: the operations reversed for a record taken reversed"""
    return "".join("%d%s" % (n, CHAR[op]) for op, n in (cg[::-1] if rev else cg))


def parse_text(s):
    """[(char, len)] of CIGAR text (H too); ValueError for anything else"""
    import re
    if not re.fullmatch(r"(\d+[IDX=H])+", s):
        raise ValueError(s)
    return [(c, int(n)) for n, c in re.findall(r"(\d+)([IDX=H])", s)]


def paf_lines(recs, rec_ops, ops, seq_len, names, read_names=None, min_block=0):
    """what `info --mappings --cigar [--names] [--min-block N]` prints: the lines of --mappings with cg:Z: appended"""
    import mappings_ref as MR
    recs = np.asarray(recs, np.uint32).reshape(-1, 12)
    out = []
    for rec, cg in zip(recs, split(rec_ops, ops)):
        if OR.block(rec) >= min_block:
            out.append(MR.paf_lines(rec[None], seq_len, names, read_names)[0] + "\tcg:Z:" + text(cg, bool(int(rec[11]) & OR.REV)))
    return out


def sam_lines(recs, rec_ops, ops, seq_len, names, read_names=None, min_block=0):
    """what `info --mappings --sam` prints"""
    import mappings_ref as MR
    recs = np.asarray(recs, np.uint32).reshape(-1, 12)
    out = ["@HD\tVN:1.6\tSO:unknown"] + ["@SQ\tSN:%s\tLN:%d" % (MR.seq_name(names, s), n) for s, n in enumerate(seq_len)]
    seen = set()
    for rec, cg in zip(recs, split(rec_ops, ops)):
        d = dict(zip(OR.FIELDS, (int(x) for x in rec)))
        later, rev = d["q"] in seen, bool(d["flags"] & OR.REV)
        seen.add(d["q"])
        if OR.block(rec) < min_block:
            continue
        head, tail = (d["qlen"] - d["qe"], d["qs"]) if rev else (d["qs"], d["qlen"] - d["qe"])
        cigar = ("%dH" % head if head else "") + text(cg, rev) + ("%dH" % tail if tail else "")
        out.append("\t".join(str(x) for x in (read_names[d["q"]] if read_names is not None else d["q"], (16 if rev else 0) | (2048 if later else 0), MR.seq_name(names, d["t"]), d["ts"] + 1, 255,
                                               cigar, "*", 0, 0, "*", "*", "NM:i:%d" % sum(n for op, n in cg if op != OP_EQ))))
    return out
