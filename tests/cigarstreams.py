"""Hand-made tuple streams for the CIGARs, over editstreams.references(), shared by the CPU suite (host twin, sanitizer program) and the
GPU suite (k_cigar_walk): the smallest shapes at which the walk with runs can go wrong — a run across the 64-byte window's edge, merging through
zero-length tuples, what is dropped in front of the first aligned column and behind the last, trailing insertions and deletions that turn interior in
a LATER window, an alt-id on the edge, and a read set whose record and operation counts make both offsets come from the scans.  Every stream is
walked by cigars_ref as it is built, and what it was made for is asserted right here."""
import numpy as np
import cigars_ref as CR
import overlaps_ref as OR
import overlapstreams as OS
from editstreams import INS, DEL, MATCH, SUBST, ANCHOR, SKIP, ALT_ID, MAIN_REF, PLAIN, START_PLAIN, START_ES, b1, b4, b5, references

ID_LIMIT = 20                                               # in the middle of the ids that read_set() uses (0, 1, 2 and 3 .. 52)


def hand_made():
    """name -> stream, every one well formed over references(); the first window holds the stream bytes 5 .. 68, the second 69 .. 132"""
    refs = references()
    S = {}

    def put(name, stream, *want, revs=None):
        got = CR.cigars_of_read(stream, refs)
        assert [CR.text(cg) for cg in got] == list(want), (name, [CR.text(cg) for cg in got])
        recs = OR.records_of_read(stream, refs)[0]
        assert CR.invariants(recs, [len(cg) for cg in got], [w for cg in got for w in CR.words(cg)]) == [], name
        if revs is not None:
            assert [r[11] & OR.REV for r in recs] == revs, name
        S[name] = stream

    ins, dl, m, x = b1(INS, 2), b1(DEL), b1(MATCH), b1(SUBST, 1)
    start = b5(START_ES, 0)
    # one operation across the window's edge: 64 of its tuples in the first window, 6 in the second
    put("run70_eq", start + m * 70, "70=")
    put("run70_x", start + x * 70, "70X")
    put("run70_ins", start + m + ins * 70 + m, "1=70I1=")      # (the run begins at the window's second tuple and crosses the edge)
    put("run70_del", start + m + dl * 70 + m, "1=70D1=")
    put("run70_eq_ends_at_the_edge", start + x * 6 + m * 58 + m * 12, "6X70=")
    # merging: through multi-byte tuples and through zero-length ones
    put("anchor_match_anchor", start + b4(ANCHOR, 10) + m + b4(ANCHOR, 5), "16=")
    put("eq_anchor0_eq", start + m + b4(ANCHOR, 0) + m, "2=")
    put("del_skip0_del", start + m + dl + b4(SKIP, 0) + dl + m, "1=2D1=")
    put("del_skip_del", start + m + dl + b4(SKIP, 7) + dl + m, "1=9D1=")
    put("ins_anchor0_ins", start + x + ins + b4(ANCHOR, 0) + ins + b4(SKIP, 0) + ins + x, "1X3I1X")
    put("anchor0_skip0_between_windows", start + m * 63 + b4(ANCHOR, 0) + b4(SKIP, 0) + m * 3, "66=")
    # what lies in front of the first aligned column is dropped: behind the start tuple, and behind an alt-id with its entry skip
    put("leading_behind_the_start", start + ins * 2 + dl + b4(SKIP, 4) + m + x, "1=1X")
    put("leading_behind_an_alt_id", start + m + b5(ALT_ID, 1) + b4(SKIP, 3) + ins + dl + m * 2, "1=", "2=")
    put("leading_fills_a_window", start + (ins + dl) * 32 + dl + ins + x + m, "1X1=")
    # ... and what lies behind the last: in front of an alt-id, in front of a main-ref, at the stream's end
    put("trailing", start + m * 2 + ins + dl + b4(SKIP, 2) + b5(ALT_ID, 1) + b4(SKIP, 1) + m + dl + b1(MAIN_REF) + m + ins * 2 + b4(SKIP, 3), "2=", "1=", "1=")
    put("trailing_fills_two_windows", start + m * 60 + (ins + dl) * 2 + (dl + ins) * 32 + ins, "60=")
    # trailing candidates that turn interior: the next aligned column lies in the NEXT window, and in the window after next
    put("interior_by_the_next_window", start + m * 60 + ins * 2 + dl * 2 + m, "60=2I2D1=")
    put("interior_runs_by_the_next_window", start + m * 58 + (ins + dl) * 3 + x + ins, "58=1I1D1I1D1I1D1X")
    put("interior_by_the_window_after_next", start + m * 60 + (ins + dl) * 2 + (dl + ins) * 32 + x + dl, "60=1I1D1I2D1I" + "1D1I" * 31 + "1X")
    put("interior_run_over_two_edges", start + m * 60 + ins * 4 + ins * 64 + ins * 2 + m + dl, "60=70I1=")
    put("interior_then_trailing_again", start + m * 62 + ins + dl + x + dl * 70 + ins, "62=1I1D1X")
    # an alt-id as the first tuple of the second window, and one that crosses the edge (it starts the second window too)
    put("alt_id_starts_the_second_window", start + m * 62 + ins + dl + b5(ALT_ID, 1) + b4(SKIP, 2) + m + x, "62=", "1=1X")
    put("alt_id_would_cross_the_edge", start + m * 61 + ins + b5(ALT_ID, 1, 1) + b4(SKIP, 2) + x + dl + m, "61=", "1X1D1=", revs=[0, 1])
    # a visit with no aligned column: no record, no operation
    put("visit_without_a_column", start + m + b5(ALT_ID, 1) + ins * 3 + dl + b5(ALT_ID, 2) + b4(SKIP, 1) + m, "1=", "1=")
    put("no_column_at_all", start + ins * 3 + dl + b4(SKIP, 2) + b4(ANCHOR, 0))
    # reversed references: the operations stay in walk order
    put("reversed_main_and_alternative", b5(START_ES, 2, 1) + b4(SKIP, 3) + m * 2 + x + dl + m + b5(ALT_ID, 1, 1) + b4(SKIP, 5) + m + ins + m + b1(MAIN_REF) + dl + x,
        "2=1X1D1=", "1=1I1=", "1X", revs=[1, 1, 1])
    # a record of one operation next to one of several hundred
    put("one_next_to_301", start + m + b1(MAIN_REF) + (m + x) * 150 + m, "1=", "1=1X" * 150 + "1=")
    return S


def read_set():
    """the read set of overlapstreams (plain reads, script reads with 0, 1 and 66 records) with the hand-made streams in between: a record's place comes
    from the scan over the reads' record counts, its operations' place from the scan over the records' operation counts"""
    out = []
    hand = list(hand_made().values())
    for i, s in enumerate(OS.read_set()):
        out.append(s)
        if i % 2 == 0:
            out.append(hand[(i // 2) % len(hand)])
    refs = references()
    rec, ops = CR.cigars(out, refs)
    assert len(rec) > 12 * 67 and rec.min() == 1 and rec.max() >= 301 and len(ops) == int(rec.sum())
    lim, _ = CR.cigars(out, refs, ID_LIMIT)                   # the limit in the middle of the ids: records of both kinds
    assert len(lim) == len(rec) and (lim == 0).sum() > 100 and (lim > 0).sum() > 100 and ((lim == 0) | (lim == rec)).all()
    return out
