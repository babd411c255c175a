"""Constructed gaps for the edit-script aligners: one read pair per case whose alignment against its reference has exactly ONE gap of a
chosen kind and shape, the table of cases (every size-class and path threshold of csrc/encode_core.hpp, align_wave.hpp, encode_es.hip),
and a planner that says from the oracle's anchors and script which aligner path the device must take.  numpy only (+ the oracle).

A pair is  ref = L + Gr + R,  read = L + Ge + R  with identical random cores L, R and gap parts whose end symbols differ, so that with
anchor length 16 the anchors are exactly (|L|, 0, 0) and (|R|, |L| + ne, |L| + nr): an inner gap of nr x ne.  Without L (or R) on both
sides the gap is the read's left (right) flank.  Adding a case: one C(...) line in CASES with the class and path it is meant to take,
then tests/golden/make_gapshapes.py (records the reference's script of the gap in tests/golden/gapshapes/cases.json)."""
import hashlib
import zlib
import numpy as np

A_LEN, K_LEN, MODULO = 16, 20, 12                 # anchor length; k and the modulo only parametrise the oracle's encoder object
ACCEPT_ALL = dict(cost_mult=2.0 ** -20, min_part_alt=1)      # every non-constant read part passes the static entropy test
PRESET = dict(cost_mult=1.0, min_part_alt=64)                # the preset's decisions
CORES = (600, 607, 608, 631)

# ---- restated from the device code ---------------------------------------------------------------------------------------------------
GK_TRIVIAL, GK_INNER, GK_FLANK, GK_FLANK_TINY = 0, 1, 2, 3
QUAD_ROWS, QUAD_CELLS, QUAD_SEQ = 1024, 32768, 2048
GIANT_ROWS, GIANT_MAX_ROWS, GIANT_WORK = 4096, 64 * 4096, 1 << 19


def gap_geometry(anchors, enc_len, ref_len, g):
    """gap g of a read with these anchors (len, pos_enc, pos_ref): dict(cur_ref, cur_enc, nr, ne, use, kind, left)  (encode_core.hpp gap_geometry)"""
    cur_ref = cur_enc = 0
    if g > 0:
        ln, pe, pr = anchors[g - 1]
        cur_ref, cur_enc = pr + ln, pe + ln
    last = g == len(anchors)
    end_enc, end_ref = enc_len, ref_len
    if not last:
        _, end_enc, end_ref = anchors[g]
    nr, ne = min(end_ref - cur_ref, ref_len - cur_ref), end_enc - cur_enc
    flank = g == 0 or last
    use = min(2 * ne, nr) if flank else nr
    if nr == 0 or ne == 0:
        kind, use = GK_TRIVIAL, 0
    elif not flank:
        kind = GK_INNER
    else:
        kind = GK_FLANK_TINY if (use < 2 or ne < 2) else GK_FLANK
    return dict(cur_ref=cur_ref, cur_enc=cur_enc, nr=nr, ne=ne, use=use, kind=kind, left=g == 0)


def gap_class(kind, use, ne):
    """(class, rows, cols)  (encode_core.hpp gap_class)"""
    if kind == GK_TRIVIAL:
        return 0, 0, 0
    rows, cols = (ne, use) if kind == GK_FLANK else (use, ne)
    if rows <= 256 and cols <= 256:
        return (rows + 63) // 64, rows, cols
    if rows <= QUAD_ROWS and rows + cols <= QUAD_SEQ and ((rows + 63) // 64) * (cols + 16) <= QUAD_CELLS:
        return 5, rows, cols
    if GIANT_ROWS < rows <= GIANT_MAX_ROWS and ((rows + 63) // 64) * cols >= GIANT_WORK and rows // 8 < cols:
        return 7, rows, cols
    return 6, rows, cols


def wave_direct_fits(n, m):
    """edlib keeps the whole history when it fits 1 MiB (align_wave.hpp wave_direct_fits)"""
    return (2 * 8 + 4) * ((n + 63) // 64) * m + 2 * 4 * m < 1024 * 1024


def quad_band(kind, rows, cols):
    """the distance up to which k_align_quad_rows keeps a class-5 gap (encode_es.hip)"""
    return (rows if kind == GK_FLANK else max(rows, cols)) // 4 + 16


def sat_rows(q, t):
    """rows a sweep of q (rows) x t (columns) computes: all, or the multiple of 64 at which t is embedded in q  (align_wave.hpp sat_rows)"""
    n, m = len(q), len(t)
    if n < m + 64:
        return n
    p = 0
    for i in range(n):
        if q[i] == t[p]:
            p += 1
            if p == m:
                return min((i // 64 + 1) * 64, n)
    return n


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def C(name, group, where, nr, ne, rel="unrelated", cls=None, path=None, **kw):
    """where: I inner, L left flank, R right flank.  rel: unrelated | disjoint (read over {A,G}, reference over {C,T}) | subs (the aligned
    parts differ by substitutions: d=<count, evenly spread> or step=<one every so many>) | dels (Ge = Gr without d evenly spread symbols)
    | subseq (Ge a random subsequence of Gr) | one (nr == 1: present=<the symbol occurs in Ge>).  cls / path: what the case is meant to take.
    Further expectations: dist, es_len, sat, minus1."""
    return dict(name=name, group=group, where=where, nr=nr, ne=ne, rel=rel, cls=cls, path=path, **kw)


def _every_where(name, group, nr, ne, rel="unrelated", cls=None, path=None, **kw):
    """an inner gap of nr x ne and both flanks with ne read symbols against nr reference symbols (rows = ne, cols = min(2 ne, nr))"""
    return [C(f"{name}_{w}", group, w, nr, ne, rel, cls, path, **kw) for w in "ILR"]


def _cases():
    out = []
    # trivial and tiny
    out += _every_where("nr0", "small", 0, 20, cls=0, path="trivial")
    out += _every_where("ne0", "small", 20, 0, cls=0, path="trivial")
    out += _every_where("use1_present", "small", 1, 30, "one", cls=1, path="small", present=True)
    out += _every_where("use1_absent", "small", 1, 30, "one", cls=1, path="small", present=False)
    out += _every_where("ne1", "small", 30, 1, cls=1, path="small")
    for nr, ne in ((14, 14), (15, 14), (14, 15), (15, 15)):
        out += _every_where(f"t{nr}x{ne}", "small", nr, ne, cls=1, path="small")
    # small classes: rows 64 / 65 ... 256 against 256 columns (a flank of r read symbols reaches 2 r reference symbols at most)
    for r in (64, 65, 128, 129, 192, 193, 256):
        out.append(C(f"s{r}x256_I", "small", "I", r, 256, "subs", (r + 63) // 64, "small", step=9))
        out.append(C(f"s{r}x256_L", "small", "L", 256, r, "subs", (r + 63) // 64, "small", step=9))
        out.append(C(f"s{r}x256_R", "small", "R", 256, r, cls=(r + 63) // 64, path="small"))
    out += [C("s257x256_I", "small", "I", 257, 256, "subs", 5, "quad", step=9), C("s256x257_I", "small", "I", 256, 257, "subs", 5, "quad", step=9),
            C("s257x256_L", "small", "L", 256, 257, "subs", 5, "quad", step=9), C("s256x257_L", "small", "L", 257, 256, "subs", 5, "quad", step=9),
            C("s257x256_R", "small", "R", 256, 257, "subs", 5, "quad", step=9), C("s256x257_R", "small", "R", 257, 256, "subs", 5, "quad", step=9)]
    # SHW "end - 1": a flank that shares nothing with the reference; a query that is no multiple of 64 symbols ends before the target starts
    for ne in (63, 64, 65, 128):
        for w in "LR":
            out.append(C(f"shw_nothing{ne}_{w}", "small", w, 300, ne, "disjoint", (ne + 63) // 64, "small", minus1=ne % 64 != 0))
    # quad
    out += [C("q1024x1024", "quad", "I", 1024, 1024, "subs", 5, "quad", step=11),
            C("q1025x1023", "quad", "I", 1025, 1023, "subs", 6, "direct", step=11),
            C("q1024x1025", "quad", "I", 1024, 1025, "subs", 6, "direct", step=11),
            C("q64x1984", "quad", "I", 64, 1984, cls=5, path="quad+redo"),
            C("q64x1985", "quad", "I", 64, 1985, cls=6, path="direct"),
            C("q400_band", "quad", "I", 400, 400, "subs", 5, "quad", d=116, dist=116),
            C("q400_band1", "quad", "I", 400, 400, "subs", 5, "quad+redo", d=117, dist=117),
            C("q400_shw_band", "quad", "L", 800, 400, "subs", 5, "quad", d=116, dist=116),
            C("q401_shw_band1", "quad", "R", 802, 401, "subs", 5, "quad+redo", d=117, dist=117),
            C("q500_unrelated", "quad", "I", 500, 500, cls=5, path="quad+redo"),
            C("q_left320", "quad", "L", 700, 320, "subs", 5, "quad", step=12), C("q_left300", "quad", "L", 700, 300, "subs", 5, "quad", step=12),
            C("q_right320", "quad", "R", 700, 320, "subs", 5, "quad", step=12), C("q_right300", "quad", "R", 700, 300, "subs", 5, "quad", step=12)]
    # wave
    out += [C("w300x9709", "wave", "I", 300, 9709, cls=6, path="direct"),
            C("w300x9710", "wave", "I", 300, 9710, cls=6, path="hirschberg"),
            C("w350x8192", "wave", "I", 350, 8192, cls=6, path="hirschberg"),    # (20 x 6 + 8) x 8192 == 1 MiB exactly: "<", not "<="
            C("w_flank1300_R", "wave", "R", 2700, 1300, "subs", 6, "sweep+direct", step=12), C("w_flank1300_L", "wave", "L", 2700, 1300, "subs", 6, "sweep+direct", step=12),
            C("w_flank1800_R", "wave", "R", 3700, 1800, "subs", 6, "hirschberg", step=12), C("w_flank1800_L", "wave", "L", 3700, 1800, "subs", 6, "hirschberg", step=12),
            C("w_rows_cols63", "wave", "I", 1063, 1000, cls=6, path="direct", sat=False), C("w_rows_cols64", "wave", "I", 1064, 1000, cls=6, path="direct", sat=False),
            C("w2000x300_subseq", "wave", "I", 2000, 300, "subseq", 6, "direct", sat=True), C("w5000x300_subseq", "wave", "I", 5000, 300, "subseq", 6, "direct", sat=True),
            C("w2000x300_nothing", "wave", "I", 2000, 300, "disjoint", 6, "direct", sat=False), C("w5000x300_nothing", "wave", "I", 5000, 300, "disjoint", 6, "direct", sat=False),
            # (a random 300-mer is embedded in a random sequence after about 4 x 300 symbols: unrelated, yet the sweep saturates)
            C("w2000x300_unrelated", "wave", "I", 2000, 300, cls=6, path="direct", sat=True), C("w5000x300_unrelated", "wave", "I", 5000, 300, cls=6, path="direct", sat=True)]
    # emission: scripts of exactly EMIT_LONG, EMIT_LONG + 1, SUM_LIMIT, SUM_LIMIT + 1 symbols
    for n, cls, path in ((256, 4, "small"), (257, 5, "quad"), (1024, 5, "quad"), (1025, 6, "direct")):
        out.append(C(f"e{n}_subs", "emit", "I", n, n, "subs", cls, path, step=9, es_len=n))
        out.append(C(f"e{n}_dels", "emit", "I", n, n - (n + 12) // 13, "dels", cls, path, d=(n + 12) // 13, es_len=n, dist=(n + 12) // 13))
    out.append(C("e700_subs", "emit", "I", 700, 700, "subs", 5, "quad", step=9, es_len=700))
    # giant thresholds
    out += [C("g4096x8200_I", "giant", "I", 4096, 8200, cls=6, path="hirschberg"), C("g4096x8192_R", "giant", "R", 8300, 4096, "subs", 6, "hirschberg", step=12),
            C("g4097x8065_I", "giant", "I", 4097, 8065, cls=6, path="hirschberg"), C("g4097x8065_L", "giant", "L", 8065, 4097, cls=6, path="hirschberg"),
            C("g4097x8066_I", "giant", "I", 4097, 8066, cls=7, path="giant"), C("g4097x8066_R", "giant", "R", 8066, 4097, "subs", 7, "giant", step=12),
            C("g16384x2048_I", "giant", "I", 16384, 2048, cls=6, path="hirschberg"), C("g16384x2048_L", "giant", "L", 2048, 16384, cls=6, path="hirschberg"),
            C("g16384x2049_I", "giant", "I", 16384, 2049, cls=7, path="giant"), C("g16384x2049_R", "giant", "R", 2049, 16384, cls=7, path="giant")]
    for c in out:                                                  # everything from the name: a new case changes no other
        c["seed"] = h = zlib.crc32(c["name"].encode())
        c["cores"] = (CORES[h % 4], CORES[(h >> 2) % 4])
        c["rc"] = (h >> 4) % 3 == 1
    return out


CASES = _cases()
GROUPS = ("small", "quad", "wave", "emit", "giant")


def group(name):
    return [c for c in CASES if c["group"] == name]


def expected_shape(c):
    """(rows, cols) as the table means them: an inner gap is nr x ne, a flank ne x min(2 ne, nr) — but use x ne when that is under 2 x 2"""
    nr, ne = c["nr"], c["ne"]
    if nr == 0 or ne == 0:
        return 0, 0
    if c["where"] == "I":
        return nr, ne
    use = min(2 * ne, nr)
    return (use, ne) if (use < 2 or ne < 2) else (ne, use)


# ---- builder -----------------------------------------------------------------------------------------------------------------------
def _other(rng, *avoid):
    return np.uint8(rng.choice([b for b in range(4) if b not in [int(a) for a in avoid]]))


def _spread(n, d):
    pos = np.unique(np.round(np.linspace(0, n - 1, d)).astype(np.int64))
    assert len(pos) == d
    return pos


def _aligned(c, rng):
    """(Gr, Ge) with the related symbols at the START of both (inner gaps and right flanks)"""
    nr, ne, rel = c["nr"], c["ne"], c["rel"]
    rnd = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    if rel == "unrelated":
        return rnd(nr), rnd(ne)
    if rel == "disjoint":
        return rng.choice(np.array([1, 3], np.uint8), nr), rng.choice(np.array([0, 2], np.uint8), ne)
    if rel == "one":
        assert nr == 1 and ne >= 3
        gr, ge = rnd(1), rnd(ne)
        ge[ge == gr[0]] = _other(rng, gr[0])
        if c["present"]:
            ge[ne // 2] = gr[0]
        return gr, ge
    if rel == "subs":
        k = min(nr, ne)
        gr = rnd(nr)
        ge = np.concatenate([gr[:k], rnd(ne - k)])
        pos = _spread(k, c["d"]) if "d" in c else np.arange(0, k, c["step"])
        ge[pos] = (ge[pos] + rng.integers(1, 4, len(pos))) % 4
        return gr, ge.astype(np.uint8)
    if rel == "dels":
        gr = rnd(nr)
        keep = np.ones(nr, bool)
        pos = _spread(nr, c["d"])
        keep[pos] = False
        assert keep.sum() == ne
        for p in pos[1:-1]:                                        # a deleted symbol that equals a neighbour would lengthen a matching run to an anchor
            gr[p] = _other(rng, gr[p - 1], gr[p + 1])
        return gr, gr[keep].copy()
    if rel == "subseq":
        gr = rnd(nr)
        pos = np.sort(rng.choice((nr - 2) // 2, ne, replace=False)) * 2 + 1          # never two neighbours, never an end
        return gr, gr[pos].copy()
    raise ValueError(rel)


def make_parts(c):
    """dict(L, R, Gr, Ge): the cores (empty where the case is a flank) and the gap's two sides, in the orientation the encoder aligns in"""
    rng = np.random.default_rng(c["seed"])
    where, nr, ne = c["where"], c["nr"], c["ne"]
    L = rng.integers(0, 4, c["cores"][0], dtype=np.uint8) if where != "L" else np.zeros(0, np.uint8)
    R = rng.integers(0, 4, c["cores"][1], dtype=np.uint8) if where != "R" else np.zeros(0, np.uint8)
    gr, ge = _aligned(c, rng)
    if where == "L":
        gr, ge = gr[::-1].copy(), ge[::-1].copy()               # related symbols next to the anchor
    # the anchors must end exactly at the gap: end symbols that differ (changing the side that keeps the case's relation intact)
    tgt, oth = (gr, ge) if c["rel"] in ("dels", "subseq") else (ge, gr)
    if nr and ne:
        for at, skip in ((0, "L"), (-1, "R")):
            if where == skip or c["rel"] == "one":
                continue
            avoid = [oth[at]] + ([oth[-1 - at]] if len(tgt) == 1 and where == "I" else [])
            if any(int(tgt[at]) == int(a) for a in avoid):
                tgt[at] = _other(rng, *avoid)
    else:
        x = ge if ne else gr                                       # one side empty: the other must not continue a core
        if len(L) and int(x[-1]) == int(L[-1]):
            x[-1] = _other(rng, L[-1], *([R[0]] if len(x) == 1 and len(R) else []))
        if len(R) and int(x[0]) == int(R[0]):
            x[0] = _other(rng, R[0], *([L[-1]] if len(x) == 1 and len(L) else []))
    return dict(L=L, R=R, Gr=gr, Ge=ge)


def make_pair(c):
    """(reference read as stored, read): the reference reverse-complemented where the case says so"""
    p = make_parts(c)
    ref = np.concatenate([p["L"], p["Gr"], p["R"]]).astype(np.uint8)
    read = np.concatenate([p["L"], p["Ge"], p["R"]]).astype(np.uint8)
    if c["rc"]:
        ref = (3 - ref[::-1]).astype(np.uint8)
    return ref, read


def expected_anchors(c):
    lL, lR = (0 if c["where"] == "L" else c["cores"][0]), (0 if c["where"] == "R" else c["cores"][1])
    out = []
    if lL:
        out.append((lL, 0, 0))
    if lR:
        out.append((lR, lL + c["ne"], lL + c["nr"]))
    return out


WHERE_CODE = {"L": 0, "I": 1, "R": 2}


def seq_sha(c):
    p = make_parts(c)
    return hashlib.sha256(bytes(p["Gr"]) + b"|" + bytes(p["Ge"]) + b"|" + bytes(p["L"]) + b"|" + bytes(p["R"])).hexdigest()


# ---- planner -----------------------------------------------------------------------------------------------------------------------
def plan_case(c):
    """The oracle's anchors and script of the case's gap, and from them the shape, class and path the device must take."""
    from oracle import pyoracle as O
    ref, read = make_pair(c)
    enc = O.Encoder(A_LEN, K_LEN, MODULO, 0, **ACCEPT_ALL)
    enc.add_ref(ref)
    cands = enc.candidates(read, [0])
    assert len(cands) == 1, f"{c['name']}: {len(cands)} candidates"
    _, rev, _, anchors = cands[0]
    oriented = (3 - ref[::-1]).astype(np.uint8) if rev else ref
    gi = {"L": 0, "I": 1, "R": len(anchors)}[c["where"]]
    classes, cells = [0] * 8, [0] * 8
    mine = None
    for g in range(len(anchors) + 1):
        geo = gap_geometry(anchors, len(read), len(ref), g)
        cls, rows, cols = gap_class(geo["kind"], geo["use"], geo["ne"])
        classes[cls] += 1
        cells[cls] += rows * cols
        if g == gi:
            mine = dict(geo, cls=cls, rows=rows, cols=cols)
    P = dict(name=c["name"], rev=int(rev), anchors=anchors, classes=classes, cells=cells, **mine)
    rp, ep = oriented[P["cur_ref"]:P["cur_ref"] + P["nr"]], read[P["cur_enc"]:P["cur_enc"] + P["ne"]]
    P["ref_part"], P["enc_part"] = rp, ep
    es, dist = O.gap_script(rp, ep, WHERE_CODE[c["where"]] if len(anchors) else 1)
    P["script"], P["dist"], P["es_len"] = es, dist, len(es)
    kind, rows, cols, cls = P["kind"], P["rows"], P["cols"], P["cls"]
    # rows (q) and columns (t) as the aligner sees them: a left flank is aligned on reversed sequences
    if kind == GK_FLANK:
        q, t = (ep[::-1], rp[::-1][:P["use"]]) if P["left"] else (ep, rp[:P["use"]])
    else:
        q, t = rp, ep                                              # (a tiny flank, also aligned reversed on the left, never reaches the wave class here)
    consumed = sum(es.count(x) for x in b"MXYZ")
    P["minus1"] = kind == GK_FLANK and consumed == 0
    P["sat"] = cls >= 6 and sat_rows(q, t) < len(q)
    P["quad_redo"] = cls == 5 and dist > quad_band(kind, rows, cols)
    if cls == 0:
        P["path"] = "trivial"
    elif cls <= 4:
        P["path"] = "small"
    elif cls == 5:
        P["path"] = "quad+redo" if P["quad_redo"] else "quad"
    elif cls == 7:
        P["path"] = "giant"
    elif kind != GK_FLANK:
        P["path"] = "direct" if wave_direct_fits(rows, cols) else "hirschberg"
    else:
        # the reference symbols the script consumes after the left flank's skipped ones: end + 1 (exact for a right flank; for a left flank
        # the canonical form may move a deletion to the front of the script, so it can be a few short: no left-flank case sits near the threshold)
        end1 = P["nr"] - (len(es) - len(es.lstrip(b"D"))) if P["left"] else sum(es.count(x) for x in b"MXYZD")
        P["end1"] = end1
        P["path"] = "direct" if wave_direct_fits(rows, cols) else "sweep+direct" if wave_direct_fits(rows, end1) else "hirschberg"
    return P


_PLANS = {}


def plan(cases):
    """plan_case of every case, computed once per process"""
    for c in cases:
        if c["name"] not in _PLANS:
            _PLANS[c["name"]] = plan_case(c)
    return [_PLANS[c["name"]] for c in cases]


def totals(plans):
    """what cl_ctx_gap_paths must report for one call over these cases: gaps per class, quad -> wave"""
    classes = [sum(p["classes"][k] for p in plans) for k in range(8)]
    return classes, sum(p["quad_redo"] for p in plans)


def total_cells(plans):
    """DP cells (rows x columns of every gap) per class of one call over these cases: what a timed context books on the aligners' launches"""
    return [sum(p["cells"][k] for p in plans) for k in range(8)]


def describe(c, p):
    return (f"{c['name']}: {c['where']} gap nr={c['nr']} ne={c['ne']} {c['rel']} rc={c['rc']} cores={c['cores']}; planned kind {p['kind']} rows {p['rows']} cols {p['cols']} "
            f"class {p['cls']} path {p['path']} sat {p['sat']} minus1 {p['minus1']} distance {p['dist']} script {p['es_len']} symbols")


def decode_tuples(t):
    """(first tuple's type, the edit script its level-0 tuples spell) of a read's tuple stream in the App. A layout"""
    out, i, first = bytearray(), 0, t[0] >> 4
    while i < len(t):
        ty, v = t[i] >> 4, t[i] & 15
        if ty in (4, 5):
            n = (v << 24) | (t[i + 1] << 16) | (t[i + 2] << 8) | t[i + 3]
            out += (b"M" if ty == 4 else b"D") * n
            i += 4
        elif ty in (6, 10):
            i += 5
        else:
            if ty <= 3:
                out.append((b"ACGT"[v], ord("D"), ord("M"), b"XYZ"[v if ty == 3 else 0])[ty])
            i += 1
    return first, bytes(out)
