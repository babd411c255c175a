"""Read-to-read overlaps from the edit scripts (cl_overlap) in plain Python, written from the definition: a read's tuples are cut
into VISITS at every alt-id / main-ref tuple, every visit is laid out as a list of its aligned COLUMNS with the read and reference positions in
front of and behind each, and a record is read off the first and the last column.  Nothing here keeps an open visit's sums in a loop the way the
kernel and the host form do.  The format and the validity checks (with their texts) are those of tests/edits_ref.py."""
import struct
import numpy as np
import edits_ref as E
from edits_ref import INS, DEL, MATCH, SUBST, ANCHOR, SKIP, ALT_ID, MAIN_REF, START_ES, Malformed

FIELDS = ("q", "t", "qlen", "tlen", "qs", "qe", "ts", "te", "matches", "subst", "anchor_bases", "flags")
REV, MAIN = 1, 2
VERSION, RECORD_BYTES = 1, 48


def visits_of(stream):
    """[(reference id, orientation nibble as written, is main, [tuples])] of an edit script: a visit opens behind start-es and behind every alt-id /
    main-ref tuple, and each of those closes the open one"""
    tup = E.tuples_of(stream)
    _, main_id, main_lo = tup[0]
    out, cur = [], (main_id, main_lo, True, [])
    for t, v, lo in tup[1:]:
        if t == ALT_ID:
            out.append(cur)
            cur = (v, lo, False, [])
        elif t == MAIN_REF:
            out.append(cur)
            cur = (main_id, main_lo, True, [])
        else:
            cur[3].append((t, v))
    out.append(cur)
    return out


def records_of_read(stream, refs, q=0, ref_read=None, read=0):
    """(the records of one read as tuples in the order of FIELDS, qlen).  Raises Malformed as edits_ref does, and for a reference id at or past the
    translation table's size."""
    stream = bytes(stream)
    E.profile_of_read(stream, refs, read)                     # every check of the profile's walk, with its text
    if stream[0] >> 4 != START_ES:
        return [], len(stream) - 1
    if ref_read is not None:
        for t, v, _ in E.tuples_of(stream):
            if t in (START_ES, ALT_ID) and v >= len(ref_read):
                raise Malformed(read, "reference id outside the reference arena")
    qpos, main_pos, first_rev, recs = 0, 0, {}, []
    for rid, lo, is_main, tuples in visits_of(stream):
        if is_main:
            rev, pos = lo != 0, main_pos
        else:
            rev, pos = first_rev.setdefault(rid, lo != 0), 0      # the orientation of the first appearance holds
        cols = []                                               # (qpos in front, reference position in front, length, type)
        for t, v in tuples:
            if t == INS:
                qpos += 1
            elif t == DEL:
                pos += 1
            elif t in (MATCH, SUBST):
                cols.append((qpos, pos, 1, t))
                qpos, pos = qpos + 1, pos + 1
            elif t == ANCHOR:
                if v > 0:
                    cols.append((qpos, pos, v, t))
                qpos, pos = qpos + v, pos + v
            elif t == SKIP:
                pos += v
        if is_main:
            main_pos = pos                                      # a main-ref comes back to where the main reference was left
        if cols:
            tlen = len(refs[rid])
            qs, ts_o = cols[0][0], cols[0][1]
            qe, te_o = cols[-1][0] + cols[-1][2], cols[-1][1] + cols[-1][2]
            anchors = sum(c[2] for c in cols if c[3] == ANCHOR)
            recs.append([q, rid if ref_read is None else int(ref_read[rid]), None, tlen, qs, qe, tlen - te_o if rev else ts_o, tlen - ts_o if rev else te_o,
                         sum(1 for c in cols if c[3] == MATCH) + anchors, sum(1 for c in cols if c[3] == SUBST), anchors, (REV if rev else 0) | (MAIN if is_main else 0)])
    if qpos > 0xffffffff:
        raise Malformed(read, "position outside the reference read")
    for r in recs:
        r[2] = qpos
    return [tuple(r) for r in recs], qpos


def records(streams, refs, first_read=0, ref_read=None):
    """the records of a batch, reads in order: an (n, 12) uint32 array; Malformed names the first bad read"""
    out = []
    for r, s in enumerate(streams):
        out += records_of_read(s, refs, first_read + r, ref_read, r)[0]
    return np.array(out, np.uint32).reshape(-1, 12)


def block(rec):
    d = dict(zip(FIELDS, (int(x) for x in rec)))
    return (d["qe"] - d["qs"]) + (d["te"] - d["ts"]) - d["matches"] - d["subst"]


def invariants(recs):
    """the relations that hold for every record, and between the records of a read; returns what is broken as (record index, name)"""
    bad, last = [], {}
    for i, rec in enumerate(np.asarray(recs, np.uint32).reshape(-1, 12)):
        d = dict(zip(FIELDS, (int(x) for x in rec)))
        checks = {"query": d["qs"] < d["qe"] <= d["qlen"], "target": d["ts"] < d["te"] <= d["tlen"], "columns": d["matches"] + d["subst"] <= min(d["qe"] - d["qs"], d["te"] - d["ts"]),
                  "anchors": d["anchor_bases"] <= d["matches"], "flags": d["flags"] < 4, "ascending": last.get(d["q"], 0) <= d["qs"], "reads_in_order": not last or d["q"] >= max(last)}
        bad += [(i, k) for k, ok in checks.items() if not ok]
        last[d["q"]] = d["qe"]
    return bad


def pack_hipoverlaps(recs, version=VERSION, record_bytes=RECORD_BYTES):
    recs = np.asarray(recs, "<u4").reshape(-1, 12)
    return struct.pack("<IIQ", version, record_bytes, len(recs)) + recs.tobytes()


def paf_lines(recs, names=None, min_block=0):
    """what `info --overlaps [--names] [--min-block N]` prints"""
    out = []
    for rec in np.asarray(recs, np.uint32).reshape(-1, 12):
        d = dict(zip(FIELDS, (int(x) for x in rec)))
        if block(rec) < min_block:
            continue
        name = (lambda i: names[i]) if names is not None else str
        out.append("\t".join(str(x) for x in (name(d["q"]), d["qlen"], d["qs"], d["qe"], "-" if d["flags"] & REV else "+", name(d["t"]), d["tlen"], d["ts"], d["te"], d["matches"],
                                               block(rec), 255, "mm:i:%d" % d["subst"], "an:i:%d" % d["anchor_bases"], "tp:A:%s" % ("P" if d["flags"] & MAIN else "S"))))
    return out
