"""GPU suite for the inverse of the edit-script encoder (csrc/expand.hip): cl_es_expand rebuilds reads from their tuple streams and the
reference reads, cl_es_verify compares the same walk with an arena.  Judges: the streams tapped from the unmodified reference (golden
es.bin) against the goldens' own reads, the plain forms, and hand-made streams whose expected bases come from the pure-Python expander
below, written from the format table of DESIGN.md section 4 (tuple type in the high nibble of the first byte; see expand_py); and the
malformed streams of tests/editstreams.py that stay inside every buffer, which both entry points must refuse."""
import numpy as np
import pytest
import torch
from util import golden
from test_gpu_dna import ref_subset, es_arrays
from colord_amd import _native as N
from colord_amd.fastq import ReadSet
import editstreams as ES

pytestmark = pytest.mark.gpu

TAPPED = ["c1_ont_default", "c2_hifi_org", "c3_clr_ratio", "c7_hifi_balanced", "s3m_ont_n_ratio", "s5m_hifi", "s4m_ont_k23_balanced"]
INS, DEL, MATCH, SUBST, ANCHOR, SKIP, ALT_ID, MAIN_REF, PLAIN, START_PLAIN, START_ES, START_PLAIN_N = range(12)


# ---- the format, in Python ----------------------------------------------------------------------------------------------------------
def tuples_of(stream: bytes):
    """(byte offset, type, value, orientation nibble) of every tuple"""
    p, out = 0, []
    while p < len(stream):
        t, lo = stream[p] >> 4, stream[p] & 0xf
        if t in (ANCHOR, SKIP):
            out.append((p, t, (lo << 24) | int.from_bytes(stream[p + 1:p + 4], "big"), 0)); p += 4
        elif t in (ALT_ID, START_ES):
            out.append((p, t, int.from_bytes(stream[p + 1:p + 5], "big"), lo)); p += 5
        else:
            out.append((p, t, lo, 0)); p += 1
    assert p == len(stream)
    return out


def expand_py(stream: bytes, refs):
    """bases (list of codes) and tuple count of one stream; refs: list of arrays of codes 0..3.  Reads no position outside a reference."""
    tup = tuples_of(stream)
    if tup[0][1] in (START_PLAIN, START_PLAIN_N):
        assert all(t == PLAIN for _, t, _, _ in tup[1:])
        return [v for _, _, v, _ in tup[1:]], len(tup)
    assert tup[0][1] == START_ES

    def at(ref, pos):
        rid, rev = ref
        r = refs[rid]
        assert 0 <= pos < len(r), "guard read"
        return int(3 - r[len(r) - 1 - pos]) if rev else int(r[pos])
    main = (tup[0][2], tup[0][3] != 0)
    cur, pos, main_pos, is_main, first_rev, out = main, 0, 0, True, {}, []
    for _, t, v, lo in tup[1:]:
        if t == INS:
            out.append(v)
        elif t == DEL:
            pos += 1
        elif t == MATCH:
            out.append(at(cur, pos)); pos += 1
        elif t == SUBST:
            rs = at(cur, pos); out.append(v + (v >= rs)); pos += 1
        elif t == ANCHOR:
            out.extend(at(cur, pos + i) for i in range(v)); pos += v
        elif t == SKIP:
            pos += v
        elif t == ALT_ID:
            if is_main:
                main_pos, is_main = pos, False
            first_rev.setdefault(v, lo != 0)            # the orientation of the first appearance holds
            cur, pos = (v, first_rev[v]), 0
        elif t == MAIN_REF:
            if not is_main:
                cur, pos, is_main = main, main_pos, True
        else:
            raise AssertionError(f"tuple type {t} inside an edit script")
    return out, len(tup)


def b1(t, lo=0): return bytes([(t << 4) | lo])
def b4(t, v): return bytes([(t << 4) | (v >> 24)]) + (v & 0xffffff).to_bytes(3, "big")
def b5(t, rid, rev): return bytes([(t << 4) | (1 if rev else 0)]) + rid.to_bytes(4, "big")


def to_device(streams, counts, device):
    raw = np.frombuffer(b"".join(streams), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    return torch.from_numpy(raw).to(device), torch.from_numpy(off).to(device), torch.from_numpy(np.asarray(counts, np.int32)).to(device)


def readset_of(seqs):
    lens = np.array([len(s) for s in seqs], np.int64)
    return ReadSet(np.concatenate([np.asarray(s, np.uint8) for s in seqs]), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), None, [], [], False)


# ---- 1. the reference's own streams -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tapped(ctx):
    """per golden: (reads arena, reference arena, device streams) made once"""
    made = {}

    def get(cfg):
        if cfg not in made:
            g = golden(cfg)
            rs = g.reads
            made[cfg] = (ctx.pack_readset(rs), ctx.pack_readset(ref_subset(rs, g.accept.astype(bool) & ~rs.has_n())), es_arrays(g, ctx.device))
        return made[cfg]
    yield get
    for reads, refs, _ in made.values():
        reads.free(); refs.free()


@pytest.mark.parametrize("cfg", TAPPED)
def test_reference_streams_expand_to_their_reads(ctx, tapped, cfg):
    rs = golden(cfg).reads
    reads, refs, (es, off, nt) = tapped(cfg)
    codes, boff = ctx.es_expand(refs, es, off, nt)
    assert np.array_equal(boff.cpu().numpy(), rs.offsets)
    assert np.array_equal(codes.cpu().numpy(), rs.bases)
    assert ctx.es_verify(reads, refs, es, off, nt) == (0, None)


# ---- 2. plain forms ---------------------------------------------------------------------------------------------------------------
def test_plain_forms_round_trip(ctx, tapped):
    rs = golden("s3m_ont_n_ratio").reads
    assert rs.has_n().any()
    reads, refs, _ = tapped("s3m_ont_n_ratio")
    es, off, nt = ctx.encode_plain(reads)
    codes, boff = ctx.es_expand(refs, es, off, nt)
    assert np.array_equal(boff.cpu().numpy(), rs.offsets) and np.array_equal(codes.cpu().numpy(), rs.bases)
    assert ctx.es_verify(reads, refs, es, off, nt) == (0, None)


# ---- 3. hand-made streams ---------------------------------------------------------------------------------------------------------
REF_LENS = (70_001, 97, 33)
ANCHOR_LENS = (1, 31, 32, 33, 63, 64, 65, 4097, 70_000)
ANCHOR_STARTS = (0, 1, 31, 32, 33)


def hand_made_streams(rng):
    S = {}
    unit = lambda: [b1(INS, int(rng.integers(4))), b1(DEL), b1(MATCH), b1(SUBST, int(rng.integers(3)))][int(rng.integers(4))]
    # one-byte tuples in runs of 55..65 (the header takes the five bytes before the first window), a 4-byte anchor, a 5-byte alt-id: the anchor
    # lies at every offset 59..64 of the window and the alt-id at every offset 59..68: both cross the window's edge at each of their bytes
    for run in range(55, 66):
        S[f"edge_run{run}"] = b5(START_ES, 0, run & 1) + b"".join(unit() for _ in range(run)) + b4(ANCHOR, 37) + b5(ALT_ID, 1 + (run & 1), run & 2) + b4(SKIP, 3) + b4(ANCHOR, 20) + \
            b1(MAIN_REF) + b"".join(unit() for _ in range(70 - run)) + b4(ANCHOR, 5)
    for rev in (0, 1):
        for a in ANCHOR_LENS:
            for p in ANCHOR_STARTS:
                if p + a <= REF_LENS[0]:
                    S[f"anchor{a}_at{p}_rev{rev}"] = b5(START_ES, 0, rev) + (b4(SKIP, p) if p else b"") + b4(ANCHOR, a)
    for first in (0, 1):      # the same alternative twice, the second time with the other orientation nibble: the first one holds
        S[f"alt_twice_first{first}"] = b5(START_ES, 0, 0) + b4(ANCHOR, 40) + b5(ALT_ID, 1, first) + b4(SKIP, 7) + b4(ANCHOR, 30) + b1(MAIN_REF) + b1(MATCH) + \
            b5(ALT_ID, 1, 1 - first) + b4(SKIP, 50) + b4(ANCHOR, 40) + b1(SUBST, 1) + b1(MAIN_REF) + b4(ANCHOR, 9)
    S["two_alternatives"] = b5(START_ES, 0, 1) + b1(MATCH) * 3 + b5(ALT_ID, 1, 0) + b4(SKIP, 2) + b4(ANCHOR, 33) + b5(ALT_ID, 2, 1) + b4(ANCHOR, 17) + b1(INS, 2) + \
        b5(ALT_ID, 1, 1) + b4(SKIP, 60) + b4(ANCHOR, 31) + b1(DEL) + b1(MATCH) + b1(MAIN_REF) + b4(ANCHOR, 64) + b5(ALT_ID, 2, 0) + b4(SKIP, 16) + b1(MATCH) * 16 + b1(MAIN_REF) + b1(SUBST, 2)
    S["start_and_one_insertion"] = b5(START_ES, 0, 0) + b1(INS, 3)
    long_units, adv = [], 0
    for _ in range(100_000):   # 100 000 one-byte tuples that stay inside reference 0
        u = unit() if adv < REF_LENS[0] else b1(INS, int(rng.integers(4)))
        adv += (u[0] >> 4) != INS
        long_units.append(u)
    S["units_100000"] = b5(START_ES, 0, 1) + b"".join(long_units)
    return S


def test_hand_made_streams(ctx):
    rng = np.random.default_rng(12)
    ref_seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in REF_LENS]
    S = hand_made_streams(rng)
    names, streams = list(S), list(S.values())
    exp = [expand_py(s, ref_seqs) for s in streams]
    assert len(exp[names.index("units_100000")][0]) > 60_000 and len(exp[names.index("anchor70000_at1_rev1")][0]) == 70_000
    refs = ctx.pack_readset(readset_of(ref_seqs))
    es, off, nt = to_device(streams, [n for _, n in exp], ctx.device)
    codes, boff = ctx.es_expand(refs, es, off, nt)
    codes, boff = codes.cpu().numpy(), boff.cpu().numpy()
    assert np.array_equal(np.diff(boff), [len(b) for b, _ in exp])
    bad = [names[i] for i, (b, _) in enumerate(exp) if not np.array_equal(codes[boff[i]:boff[i + 1]], np.asarray(b, np.uint8))]
    assert not bad, bad
    reads = ctx.pack_readset(readset_of([np.asarray(b, np.uint8) for b, _ in exp]))
    assert ctx.es_verify(reads, refs, es, off, nt) == (0, None)
    reads.free(); refs.free()


# ---- 4. what must be reported -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last", "word_boundary"])
@pytest.mark.parametrize("kind", ["edit_script", "plain"])
def test_one_changed_input_base_is_one_bad_read(ctx, tapped, where, kind):
    g = golden("c3_clr_ratio" if kind == "edit_script" else "s3m_ont_n_ratio")
    rs = g.reads
    _, refs, (es, off, nt) = tapped(g.cfg)
    want = START_ES if kind == "edit_script" else START_PLAIN_N
    i = next(r for r in range(rs.n_reads // 2, rs.n_reads) if g.es[r][2][0] >> 4 == want and len(rs.read(r)) > 64)
    at = {"first": 0, "last": len(rs.read(i)) - 1, "word_boundary": 32}[where]
    bases = rs.bases.copy()
    b = bases[rs.offsets[i] + at]
    bases[rs.offsets[i] + at] = (b + 1) % 4 if b < 4 else 0
    changed = ctx.pack_reads(torch.from_numpy(bases), torch.from_numpy(rs.offsets))
    assert ctx.es_verify(changed, refs, es, off, nt) == (1, i)
    changed.free()


def test_one_changed_insertion_is_one_bad_read(ctx, tapped):
    g = golden("c3_clr_ratio")
    reads, refs, _ = tapped(g.cfg)
    i, at = next((r, p) for r in range(g.reads.n_reads // 3, g.reads.n_reads) if g.es[r][2][0] >> 4 == START_ES for p, t, _, _ in tuples_of(g.es[r][2])[1:] if t == INS)
    streams = [e[2] for e in g.es]
    s = bytearray(streams[i])
    s[at] = (INS << 4) | ((s[at] & 0xf) + 1) % 4
    streams[i] = bytes(s)
    es, off, nt = to_device(streams, [e[1] for e in g.es], ctx.device)
    assert ctx.es_verify(reads, refs, es, off, nt) == (1, i)


# ---- 5. malformed streams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ES.malformed_device()))
def test_malformed_stream_is_refused(ctx, name):
    """the malformed streams the profile and the overlaps take (they lie inside every buffer whether or not a check were missing), as read 0
    next to a well-formed read 1: both entry points refuse the call and name the read and what it ran into; the well-formed one alone passes"""
    bad, why = ES.malformed_device()[name]
    ref_seqs = ES.references()
    good = ES.b5(START_ES, 0, 1) + ES.b1(MATCH) * 3 + ES.b4(ANCHOR, 40) + ES.b5(ALT_ID, 1) + ES.b4(SKIP, 2) + ES.b4(ANCHOR, 33) + ES.b1(MAIN_REF) + ES.b1(SUBST, 1) + ES.b1(INS, 2)
    bases, ntup = expand_py(good, ref_seqs)
    refs = ctx.pack_readset(readset_of(ref_seqs))
    both = ctx.pack_readset(readset_of([np.zeros(4, np.uint8), np.asarray(bases, np.uint8)]))
    es, off, _ = to_device([bad, good], [0, ntup], ctx.device)
    for call in (lambda: ctx.es_expand(refs, es, off), lambda: ctx.es_verify(both, refs, es, off)):
        with pytest.raises(N.ColordHipError) as x:
            call()
        assert x.value.status == N.CL_E_INVALID and "read 0: " + why in str(x.value), str(x.value)
    alone = ctx.pack_readset(readset_of([np.asarray(bases, np.uint8)]))
    es, off, nt = to_device([good], [ntup], ctx.device)
    codes, boff = ctx.es_expand(refs, es, off, nt)
    assert boff.cpu().numpy().tolist() == [0, len(bases)] and codes.cpu().numpy().tolist() == bases
    assert ctx.es_verify(alone, refs, es, off, nt) == (0, None)
    refs.free(); both.free(); alone.free()
