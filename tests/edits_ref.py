"""The edit-operation profile (cl_edits) in plain Python, written from the format table of DESIGN.md 4d — the tuple type in the
high nibble of the first byte; one byte: ins, del, match, subst, main-ref, plain and the two start-plain forms; four bytes: anchor and skip
(28-bit big-endian value); five bytes: alt-id and start-es (low nibble = orientation, 32-bit big-endian id) — and from the definitions of the
fields.  A read is first turned into a list of EVENTS (type, value, reference base under the cursor), then every field is counted from the
events with groupby / Counter; nothing here walks a window or keeps a counter in a loop the way the kernel and the host form do."""
from collections import Counter
from itertools import groupby
import numpy as np

INS, DEL, MATCH, SUBST, ANCHOR, SKIP, ALT_ID, MAIN_REF, PLAIN, START_PLAIN, START_ES, START_PLAIN_N = range(12)
SIZE = {ANCHOR: 4, SKIP: 4, ALT_ID: 5, START_ES: 5}
FIELDS = (("reads", 0), ("bases", 0), ("kind_reads", 3), ("kind_bases", 3), ("kind_bytes", 3), ("main_rev", 2), ("tuples", 8), ("anchor_bases", 0), ("anchor_len_hist", 29),
          ("skip_entries", 0), ("skip_entry_sum", 0), ("skip_bases", 0), ("skip_len_hist", 29), ("ins_base", 4), ("del_base", 4), ("match_base", 4), ("sub", (4, 4)),
          ("ins_run_hist", 17), ("del_run_hist", 17), ("identity_hist", 101), ("identity_none", 0), ("alt_hist", 65))
WORDS = sum(int(np.prod(s)) if s else 1 for _, s in FIELDS)


class Malformed(Exception):
    def __init__(self, read, why):
        super().__init__(f"read {read}: {why}")
        self.read, self.why = read, why


def empty():
    return {k: (np.zeros(s, np.uint64) if s else 0) for k, s in FIELDS}


def add(a, b):
    return {k: a[k] + b[k] for k, _ in FIELDS}


def same(a, b, fields=None):
    """None, or the name of the first field that differs"""
    for k, s in FIELDS:
        if fields is None or k in fields:
            if (not np.array_equal(np.asarray(a[k], np.uint64), np.asarray(b[k], np.uint64))) if s else int(a[k]) != int(b[k]):
                return k
    return None


def flat(e):
    """the WORDS counters in the order of cl_edits"""
    return [int(x) for k, s in FIELDS for x in (np.asarray(e[k]).reshape(-1) if s else [e[k]])]


def unflat(words):
    e, at = empty(), 0
    for k, s in FIELDS:
        n = int(np.prod(s)) if s else 1
        e[k] = np.array(words[at:at + n], np.uint64).reshape(s) if s else int(words[at])
        at += n
    return e


def pack_hipedits(e, version=1, flags=0):
    return np.array([version, flags], "<u4").tobytes() + np.array(flat(e), "<u8").tobytes()


def unpack_hipedits(b):
    assert len(b) == 8 + 8 * WORDS and tuple(np.frombuffer(b[:8], "<u4")) == (1, 0)
    return unflat([int(x) for x in np.frombuffer(b[8:], "<u8")])


def hist(values, n):
    return np.bincount(np.asarray(values, np.int64), minlength=n).astype(np.uint64)


def tuples_of(stream, read=0):
    """[(type, value, low nibble)] of a stream; a tuple that crosses its end is malformed"""
    p, out, n = 0, [], len(stream)
    while p < n:
        t, lo = stream[p] >> 4, stream[p] & 0xf
        size = SIZE.get(t, 1)
        if p + size > n:
            raise Malformed(read, "tuple crosses the end of the stream")
        if size == 4:
            out.append((t, (lo << 24) | int.from_bytes(stream[p + 1:p + 4], "big"), lo))
        elif size == 5:
            out.append((t, int.from_bytes(stream[p + 1:p + 5], "big"), lo))
        else:
            out.append((t, lo, lo))
        p += size
    return out


def events_of(stream, refs, read=0):
    """An edit script as events (type, value, reference base under the cursor or None), the orientation of the main reference and the distinct
    alternatives.  refs: sequences of codes 0..3.  Reads no position outside a reference: such a script is malformed."""
    tup = tuples_of(stream, read)
    _, main_id, main_lo = tup[0]
    if main_id >= len(refs):
        raise Malformed(read, "reference id outside the reference arena")

    def under(where):
        (rid, rev), pos = where
        r = refs[rid]
        if not 0 <= pos < len(r):
            raise Malformed(read, "position outside the reference read")
        return 3 - int(r[len(r) - 1 - pos]) if rev else int(r[pos])
    main = (main_id, main_lo != 0)
    cur, pos, left_main_at, first_rev, ev = main, 0, None, {}, []
    for t, v, lo in tup[1:]:
        if t > MAIN_REF:
            raise Malformed(read, "tuple type not allowed inside an edit script")
        if t == INS and v > 3 or t == SUBST and v > 2:
            raise Malformed(read, "base value out of range")
        ev.append((t, v, under((cur, pos)) if t in (DEL, MATCH, SUBST) else None))
        if t in (DEL, MATCH, SUBST):
            pos += 1
        elif t == ANCHOR:
            if pos + v > len(refs[cur[0]]):
                raise Malformed(read, "position outside the reference read")
            pos += v
        elif t == SKIP:
            pos += v
        elif t == ALT_ID:
            if v >= len(refs):
                raise Malformed(read, "reference id outside the reference arena")
            if left_main_at is None:
                left_main_at = pos
            if v not in first_rev and len(first_rev) == 64:
                raise Malformed(read, "more than 64 alternative references")
            first_rev.setdefault(v, lo != 0)                # the orientation of the first appearance holds
            cur, pos = (v, first_rev[v]), 0
        elif t == MAIN_REF and left_main_at is not None:
            cur, pos, left_main_at = main, left_main_at, None
    return ev, main[1], len(first_rev)


def profile_of_read(stream, refs, read=0):
    e = empty()
    n = len(stream)
    if n == 0:
        raise Malformed(read, "empty stream")
    first = stream[0] >> 4
    if first in (START_PLAIN, START_PLAIN_N):
        if any(b >> 4 != PLAIN for b in stream[1:]):
            raise Malformed(read, "tuple type not allowed inside an edit script")
        if any(b & 0xf > 4 for b in stream[1:]):
            raise Malformed(read, "base value out of range")
        kind, bases = (0 if first == START_PLAIN else 1), n - 1
    elif first != START_ES:
        raise Malformed(read, "first tuple is no start tuple")
    else:
        ev, rev, n_alt = events_of(stream, refs, read)
        kind = 2
        types = [t for t, _, _ in ev]
        by_type = Counter(types)
        e["tuples"] = np.array([by_type[t] for t in range(8)], np.uint64)
        anchors = [v for t, v, _ in ev if t == ANCHOR]
        entries = [v for i, (t, v, _) in enumerate(ev) if t == SKIP and i > 0 and types[i - 1] == ALT_ID]
        skips = [v for i, (t, v, _) in enumerate(ev) if t == SKIP and not (i > 0 and types[i - 1] == ALT_ID)]
        e["anchor_bases"], e["skip_entries"], e["skip_entry_sum"], e["skip_bases"] = sum(anchors), len(entries), sum(entries), sum(skips)
        e["anchor_len_hist"] = hist([v.bit_length() for v in anchors], 29)
        e["skip_len_hist"] = hist([v.bit_length() for v in skips], 29)
        e["ins_base"] = hist([v for t, v, _ in ev if t == INS], 4)
        e["del_base"] = hist([rb for t, _, rb in ev if t == DEL], 4)
        e["match_base"] = hist([rb for t, _, rb in ev if t == MATCH], 4)
        for (frm, to), c in Counter((rb, v + (v >= rb)) for t, v, rb in ev if t == SUBST).items():
            e["sub"][frm, to] = c
        for t, grp in groupby(types):
            if t in (INS, DEL):
                e["ins_run_hist" if t == INS else "del_run_hist"][min(len(list(grp)), 16)] += np.uint64(1)
        m = by_type[MATCH] + sum(anchors)
        d = m + by_type[SUBST] + by_type[INS] + by_type[DEL]
        if d:
            e["identity_hist"][100 * m // d] = 1
        else:
            e["identity_none"] = 1
        e["alt_hist"][n_alt] = 1
        e["main_rev"][int(rev)] = 1
        bases = by_type[INS] + by_type[MATCH] + by_type[SUBST] + sum(anchors)
    e["kind_reads"][kind], e["kind_bases"][kind], e["kind_bytes"][kind] = 1, bases, n
    e["reads"], e["bases"] = 1, bases
    return e


def profile(streams, refs):
    """the profile of a batch: streams = byte strings, refs = sequences of codes 0..3; Malformed names the first bad read"""
    words = np.zeros(WORDS, object)
    for r, s in enumerate(streams):
        words += np.array(flat(profile_of_read(bytes(s), refs, r)), object)
    return unflat([int(x) for x in words])


def invariants(e):
    """the relations of DESIGN.md 4i that hold for every profile; returns the names of those that do not"""
    t = [int(x) for x in e["tuples"]]
    checks = {
        "kind_bases": int(np.sum(e["kind_bases"])) == e["bases"], "kind_reads": int(np.sum(e["kind_reads"])) == e["reads"],
        "script_bases": t[INS] + t[MATCH] + t[SUBST] + e["anchor_bases"] == int(e["kind_bases"][2]),
        "sub_diagonal": not np.diag(e["sub"]).any(), "sub": int(np.sum(e["sub"])) == t[SUBST], "ins_base": int(np.sum(e["ins_base"])) == t[INS],
        "del_base": int(np.sum(e["del_base"])) == t[DEL], "match_base": int(np.sum(e["match_base"])) == t[MATCH],
        "anchor_len_hist": int(np.sum(e["anchor_len_hist"])) == t[ANCHOR], "skips": e["skip_entries"] + int(np.sum(e["skip_len_hist"])) == t[SKIP],
        "identity": int(np.sum(e["identity_hist"])) + e["identity_none"] == int(e["kind_reads"][2]), "alt_hist": int(np.sum(e["alt_hist"])) == int(e["kind_reads"][2]),
        "main_rev": int(np.sum(e["main_rev"])) == int(e["kind_reads"][2]), "run_index_0": e["ins_run_hist"][0] == 0 and e["del_run_hist"][0] == 0,
    }
    return [k for k, ok in checks.items() if not ok]
