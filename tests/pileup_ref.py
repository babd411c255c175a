"""The judge of the pileup, in plain Python with numpy and written from the definition: the walk of the tuple streams with what
every tuple books, the fold, the sites, the totals, the `hippileup` stream, and what `colord_hip info --pileup` prints.  Nothing here is shared
with the code under test."""
import struct
import numpy as np

INS, DEL, MATCH, SUBST, ANCHOR, SKIP, ALT_ID, MAIN_REF, PLAIN, START_PLAIN, START_ES, START_PLAIN_N = range(12)
COLS = ("match", "subA", "subC", "subG", "subT", "del", "ins", "ref")
C_MATCH, C_SUB, C_DEL, C_INS, C_REF = 0, 1, 5, 6, 7
SITE_FIELDS = ("seq", "pos", "ref", "kind", "match", "subA", "subC", "subG", "subT", "del", "ins", "depth")
TOTALS = ("covered", "match", "sub", "del", "ins", "ins_unplaced", "reads")
KINDS = ("A", "C", "G", "T", "del", "ins")
DEFAULTS = (4, 3, 250)
VERSION, RECORD_BYTES, HEAD = 1, 48, 32 + 56 + 8
M32 = 1 << 32


def pieces(seq_len, read_len, overlap):
    """(sequence, start, length) of every piece in the order of their ids: a piece every read_len - overlap bases of every sequence"""
    assert read_len > overlap
    out = []
    for s, ln in enumerate(seq_len):
        start = 0
        while start < ln:
            out.append((s, start, min(read_len, ln - start)))
            start += read_len - overlap
    return out


def cut(seqs, read_len, overlap):
    """the pieces of the sequences as arrays: the pseudo reads"""
    return [np.asarray(seqs[s][a:a + ln], np.uint8) for s, a, ln in pieces([len(x) for x in seqs], read_len, overlap)]


class Table:
    """the table of a genome: per position the eight counters, the anchors' difference array, the totals"""

    def __init__(self, seqs, read_len, overlap):
        self.seqs = [np.asarray(s, np.uint8) for s in seqs]
        self.seq_len = [len(s) for s in self.seqs]
        self.read_len, self.overlap = read_len, overlap
        self.base = np.concatenate([[0], np.cumsum(self.seq_len)]).astype(np.int64)
        self.n_pos = int(self.base[-1])
        assert self.n_pos < M32
        self.P = pieces(self.seq_len, read_len, overlap)
        self.n_pseudo = len(self.P)
        self.origin = [int(self.base[s]) + a for s, a, _ in self.P]
        self.cols = np.zeros((self.n_pos, 8), np.int64)
        self.diff = np.zeros(self.n_pos + 1, np.int64)
        self.t = dict.fromkeys(TOTALS, 0)
        self.folded = False

    def add(self, streams, refs):
        """refs: the reference reads the streams point to, the pieces first"""
        for i, (s, a, ln) in enumerate(self.P):
            assert len(refs[i]) == ln
        for st in streams:
            self._read(bytes(st), refs)

    def _read(self, s, refs):
        t0 = s[0] >> 4
        if t0 in (START_PLAIN, START_PLAIN_N):
            return
        assert t0 == START_ES and len(s) >= 5
        ident = lambda at: int.from_bytes(s[at + 1:at + 5], "big")
        main = (ident(0), bool(s[0] & 0xf))
        cur, cursor, main_cursor, on_main = main, 0, 0, True
        alts, last_ins, touched, at = {}, False, False, 5
        while at < len(s):
            t, v = s[at] >> 4, s[at] & 0xf
            rid, rev = cur
            ln = len(refs[rid])
            genome = rid < self.n_pseudo
            o = self.origin[rid] if genome else None
            fwd = lambda c: o + (ln - 1 - c if rev else c)
            if t <= SKIP and genome:
                touched = True
            if t == INS:
                assert v <= 3
                if genome and not last_ins:
                    if rev and cursor < ln:
                        self.cols[fwd(cursor), C_INS] += 1
                    elif not rev and 1 <= cursor <= ln:
                        self.cols[fwd(cursor - 1), C_INS] += 1
                    else:
                        self.t["ins_unplaced"] += 1
                at += 1
            elif t in (DEL, MATCH, SUBST):
                assert cursor < ln, "position outside the reference read"
                if genome:
                    if t == DEL:
                        self.cols[fwd(cursor), C_DEL] += 1
                    elif t == MATCH:
                        self.cols[fwd(cursor), C_MATCH] += 1
                    else:
                        assert v <= 2
                        rb = int(refs[rid][ln - 1 - cursor]) ^ 3 if rev else int(refs[rid][cursor])        # the reference base as the stream sees it
                        b = v + (1 if v >= rb else 0)                                                       # the read's base, stream orientation
                        self.cols[fwd(cursor), C_SUB + (3 - b if rev else b)] += 1
                cursor += 1; at += 1
            elif t in (ANCHOR, SKIP):
                val = (v << 24) | int.from_bytes(s[at + 1:at + 4], "big")
                if t == ANCHOR:
                    assert cursor + val <= ln, "position outside the reference read"
                    if genome and val:
                        a = o + (ln - cursor - val if rev else cursor)
                        self.diff[a] += 1; self.diff[a + val] -= 1
                cursor += val; at += 4
            elif t == ALT_ID:
                rid2 = ident(at)
                if rid2 not in alts:
                    assert len(alts) < 64
                    alts[rid2] = bool(v)
                if on_main:
                    main_cursor, on_main = cursor, False
                cur, cursor = (rid2, alts[rid2]), 0
                at += 5
            else:
                assert t == MAIN_REF
                if not on_main:
                    cur, cursor, on_main = main, main_cursor, True
                at += 1
            last_ins = t == INS
        assert at == len(s)
        self.t["reads"] += 1 if touched else 0

    def fold(self):
        assert not self.folded
        self.folded = True
        self.cols[:, C_MATCH] += np.cumsum(self.diff)[:self.n_pos]
        assert (self.cols >= 0).all() and (self.cols < M32).all()
        if self.n_pos:
            self.cols[:, C_REF] = np.concatenate(self.seqs)
        c = self.cols
        depth = c[:, 0] + c[:, 1:5].sum(1) + c[:, 5]
        self.t.update(covered=int((depth >= 1).sum()), match=int(c[:, 0].sum()), sub=int(c[:, 1:5].sum()), **{"del": int(c[:, 5].sum())}, ins=int(c[:, 6].sum()))
        return self

    def columns(self):
        return self.cols.astype(np.uint32)

    def totals(self):
        return dict(self.t)

    def sites(self, min_depth=4, min_alt=3, min_permille=250):
        return sites_of(self.cols, self.base, min_depth, min_alt, min_permille)


def alt_of(col):
    """(alt, kind) of a position's counters: the largest of sub[b] for b != ref, del and ins; ties to the lowest kind"""
    ref = int(col[C_REF])
    cand = [(int(col[C_SUB + b]), b) for b in range(4) if b != ref] + [(int(col[C_DEL]), 4), (int(col[C_INS]), 5)]
    best = max(v for v, _ in cand)
    return best, min(k for v, k in cand if v == best)


def sites_of(cols, base, min_depth, min_alt, min_permille):
    cols = np.asarray(cols, np.int64)
    depth = cols[:, 0] + cols[:, 1:5].sum(1) + cols[:, 5]
    cand = cols[:, 1:7].copy()
    cand[np.arange(len(cols)), cols[:, C_REF]] = -1                        # the reference's own base is no alternative
    alt, kind = cand.max(1), cand.argmax(1)                                # (the first of equal values: ties go to the lowest kind)
    out = []
    for x in np.nonzero((depth >= min_depth) & (alt >= min_alt) & (alt * 1000 >= min_permille * depth))[0]:
        assert (int(alt[x]), int(kind[x])) == alt_of(cols[x])
        s = int(np.searchsorted(base, x, side="right")) - 1
        out.append((s, int(x - base[s]), int(cols[x, C_REF]), int(kind[x])) + tuple(int(v) for v in cols[x, :7]) + (int(depth[x]),))
    return np.array(out, np.uint32).reshape(-1, 12)


# ---- the `hippileup` stream ---------------------------------------------------------------------------------------------------------------
def pack(sites, seq_len, names, read_len, overlap, thresholds, totals, version=VERSION, record_bytes=RECORD_BYTES, count=None):
    sites = np.asarray(sites, "<u4").reshape(-1, 12)
    b = struct.pack("<8I", version, record_bytes, len(seq_len), read_len, overlap, *thresholds) + struct.pack("<7Q", *(totals[k] for k in TOTALS))
    b += struct.pack("<Q", len(sites) if count is None else count)
    for ln, nm in zip(seq_len, names):
        nm = nm.encode() if isinstance(nm, str) else nm
        b += struct.pack("<QH", ln, len(nm)) + nm
    return b + sites.tobytes()


def parse(b):
    """-> dict; ValueError for everything the stream's reader must refuse"""
    if len(b) < HEAD:
        raise ValueError("head")
    version, rb, n_seqs, read_len, overlap, d, a, pm = struct.unpack_from("<8I", b, 0)
    if version != VERSION or rb != RECORD_BYTES:
        raise ValueError("version or record size")
    totals = dict(zip(TOTALS, struct.unpack_from("<7Q", b, 32)))
    count, = struct.unpack_from("<Q", b, 88)
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
    sites = np.frombuffer(b, "<u4", offset=at).reshape(-1, 12).astype(np.uint32)
    last = (-1, -1)
    for r in sites:
        if r[0] >= n_seqs or r[1] >= seq_len[r[0]] or r[2] > 3 or r[3] > 5 or r[3] == r[2]:
            raise ValueError("site")
        if (int(r[0]), int(r[1])) <= last:
            raise ValueError("order")
        last = (int(r[0]), int(r[1]))
    return dict(seq_len=seq_len, names=names, read_len=read_len, overlap=overlap, thresholds=(d, a, pm), totals=totals, sites=sites)


def seq_name(names, s):
    return names[s] if names[s] else str(s)


def alt_count(r):
    return int(r[5 + r[3]]) if r[3] < 4 else int(r[9 + (r[3] - 4)])


def kept(sites, min_alt=0, min_permille=0):
    """the sites that pass thresholds given to `info`, which can only tighten what was stored"""
    return [r for r in np.asarray(sites, np.uint32).reshape(-1, 12) if alt_count(r) >= min_alt and alt_count(r) * 1000 >= min_permille * int(r[11])]


def base_counts(r):
    """A, C, G, T of a site: the reference base's column is `match`"""
    return [int(r[4]) if b == r[2] else int(r[5 + b]) for b in range(4)]


def tsv_lines(sites, names, min_alt=0, min_permille=0):
    """what `info --pileup [--min-alt N] [--min-frac F]` prints"""
    return ["\t".join(str(x) for x in [seq_name(names, int(r[0])), int(r[1]) + 1, "ACGT"[r[2]], int(r[11])] + base_counts(r) + [int(r[9]), int(r[10]), KINDS[r[3]]])
            for r in kept(sites, min_alt, min_permille)]


def vcf_lines(sites, seq_len, names, min_alt=0, min_permille=0):
    """what `info --pileup --vcf` prints: the sites whose kind is a base"""
    out = ["##fileformat=VCFv4.2", "##source=colord_hip"] + ["##contig=<ID=%s,length=%d>" % (seq_name(names, s), ln) for s, ln in enumerate(seq_len)]
    out += ['##INFO=<ID=DP,Number=1,Type=Integer,Description="Aligned columns at the position: match + substitutions + deletions">',
            '##INFO=<ID=AD,Number=R,Type=Integer,Description="Columns that say the reference base, columns that say the alternative">',
            '##INFO=<ID=AF,Number=A,Type=Float,Description="Alternative columns over DP">',
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    for r in kept(sites, min_alt, min_permille):
        if r[3] < 4:
            alt, dp = alt_count(r), int(r[11])
            out.append("%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;AD=%d,%d;AF=%.4f" % (seq_name(names, int(r[0])), int(r[1]) + 1, "ACGT"[r[2]], "ACGT"[r[3]], dp, int(r[4]), alt, alt / dp if dp else 0.0))
    return out


def summary(S):
    """what `info --pileup --summary --json` prints, as a dict (S: what parse() gives)"""
    t = S["totals"]
    cols = t["match"] + t["sub"] + t["del"]
    r6 = lambda a, b: float("%.6f" % (a / b if b else 0.0))
    by = {k: 0 for k in KINDS}
    for r in S["sites"]:
        by[KINDS[r[3]]] += 1
    return {"sequences": len(S["seq_len"]), "positions": int(sum(S["seq_len"])), "min_depth": S["thresholds"][0], "min_alt": S["thresholds"][1], "min_permille": S["thresholds"][2],
            "covered": t["covered"], "match": t["match"], "sub": t["sub"], "del": t["del"], "ins": t["ins"], "ins_unplaced": t["ins_unplaced"], "reads": t["reads"],
            "mean_depth": r6(cols, t["covered"]), "sub_rate": r6(t["sub"], cols), "del_rate": r6(t["del"], cols), "ins_rate": r6(t["ins"], cols),
            "sites": len(S["sites"]), "sites_by_kind": by}
