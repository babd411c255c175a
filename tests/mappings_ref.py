"""The judge of the read-to-genome mappings, in plain Python and written from the definition: the geometry of the genome's pieces,
the lift of overlap records (tests/overlaps_ref.py has the record) to the genome's sequences, the `hipmappings` stream, and what `colord_hip info
--mappings` prints.  Nothing here is shared with the code under test."""
import struct
import numpy as np
import overlaps_ref as OR

FIELDS = OR.FIELDS
GENOME = 4                                  # flags bit 2: a target in genome coordinates
VERSION, RECORD_BYTES, HEAD = 1, 48, 28
TLEN, POS, END = 1, 2, 3                    # what refuses a record, in the order of the checks
POS_MAX = 0xffffffff


class Refused(Exception):
    def __init__(self, record, code):
        super().__init__("record %d: code %d" % (record, code))
        self.record, self.code = record, code


def pieces(seq_len, read_len, overlap):
    """(sequence, start, length) of every piece, in the order of their ids: a piece every read_len - overlap bases of every sequence"""
    assert read_len > overlap
    out = []
    for s, ln in enumerate(seq_len):
        start = 0
        while start < ln:
            out.append((s, start, min(read_len, ln - start)))
            start += read_len - overlap
    return out


def lift(recs, seq_len, read_len, overlap):
    """the records whose target is a piece, moved to their sequence, in their order; Refused names the first record that cannot be"""
    P = pieces(seq_len, read_len, overlap)
    out = []
    for i, rec in enumerate(np.asarray(recs, np.uint32).reshape(-1, 12)):
        d = dict(zip(FIELDS, (int(x) for x in rec)))
        if d["t"] >= len(P):
            continue
        s, start, ln = P[d["t"]]
        if d["tlen"] != ln:
            raise Refused(i, TLEN)
        if start + d["ts"] > POS_MAX or start + d["te"] > POS_MAX:
            raise Refused(i, POS)
        if start + d["te"] > seq_len[s]:
            raise Refused(i, END)
        d.update(t=s, tlen=seq_len[s], ts=start + d["ts"], te=start + d["te"], flags=d["flags"] | GENOME)
        out.append(tuple(d[k] for k in FIELDS))
    return np.array(out, np.uint32).reshape(-1, 12)


def pack(recs, seq_len, names, read_len, overlap, version=VERSION, record_bytes=RECORD_BYTES, count=None):
    recs = np.asarray(recs, "<u4").reshape(-1, 12)
    b = struct.pack("<IIIIIQ", version, record_bytes, len(seq_len), read_len, overlap, len(recs) if count is None else count)
    for ln, nm in zip(seq_len, names):
        nm = nm.encode() if isinstance(nm, str) else nm
        b += struct.pack("<QH", ln, len(nm)) + nm
    return b + recs.tobytes()


def parse(b):
    """-> (seq_len, names, read_len, overlap, records); ValueError for everything the stream's reader must refuse"""
    if len(b) < HEAD:
        raise ValueError("head")
    version, rb, n_seqs, read_len, overlap, count = struct.unpack_from("<IIIIIQ", b, 0)
    if version != VERSION or rb != RECORD_BYTES:
        raise ValueError("version or record size")
    at, seq_len, names = HEAD, [], []
    for _ in range(n_seqs):
        if len(b) - at < 10:
            raise ValueError("name table")
        ln, nl = struct.unpack_from("<QH", b, at)
        at += 10
        if len(b) - at < nl:
            raise ValueError("name table")
        seq_len.append(ln); names.append(b[at:at + nl].decode()); at += nl
    if len(b) - at != count * RECORD_BYTES:
        raise ValueError("count")
    recs = np.frombuffer(b, "<u4", offset=at).reshape(-1, 12).astype(np.uint32)
    for r in recs:
        if r[1] >= n_seqs or r[7] > seq_len[r[1]]:
            raise ValueError("record")
    return seq_len, names, read_len, overlap, recs


def seq_name(names, s):
    return names[s] if names[s] else str(s)


def paf_lines(recs, seq_len, names, read_names=None, min_block=0):
    """what `info --mappings [--names] [--min-block N]` prints"""
    out = []
    for rec in np.asarray(recs, np.uint32).reshape(-1, 12):
        d = dict(zip(FIELDS, (int(x) for x in rec)))
        if OR.block(rec) < min_block:
            continue
        q = read_names[d["q"]] if read_names is not None else str(d["q"])
        out.append("\t".join(str(x) for x in (q, d["qlen"], d["qs"], d["qe"], "-" if d["flags"] & OR.REV else "+", seq_name(names, d["t"]), seq_len[d["t"]], d["ts"], d["te"], d["matches"],
                                               OR.block(rec), 255, "mm:i:%d" % d["subst"], "an:i:%d" % d["anchor_bases"], "tp:A:%s" % ("P" if d["flags"] & OR.MAIN else "S"))))
    return out


def coverage_lines(recs, seq_len, names, window):
    """what `info --mappings --coverage W` prints: per window the target bases of the records in it over its length"""
    out = []
    recs = np.asarray(recs, np.uint32).reshape(-1, 12).astype(np.int64)
    for s, ln in enumerate(seq_len):
        mine = recs[recs[:, 1] == s]
        for a in range(0, ln, window):
            e = min(a + window, ln)
            inside = int(np.clip(np.minimum(mine[:, 7], e) - np.maximum(mine[:, 6], a), 0, None).sum())
            out.append("%s\t%d\t%d\t%.6f" % (seq_name(names, s), a, e, inside / (e - a)))
    return out


def summary(recs, n_reads):
    """what `info --mappings --summary --json` prints, as a dict"""
    recs = np.asarray(recs, np.uint32).reshape(-1, 12)
    hist = [0] * 101
    for rec in recs:
        blk = OR.block(rec)
        hist[100 * min(int(rec[8]), blk) // blk if blk else 0] += 1
    rev = int(sum(1 for r in recs if r[11] & OR.REV))
    return {"reads": n_reads, "reads_mapped": len(set(recs[:, 0].tolist())), "records": len(recs), "aligned_query_bases": int((recs[:, 5].astype(np.int64) - recs[:, 4]).sum()),
            "forward": len(recs) - rev, "reverse": rev, "identity_hist": hist}
