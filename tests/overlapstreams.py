"""Hand-made tuple streams for the overlap records, over editstreams.references(), shared by the CPU suite (host form, sanitizer
program) and the GPU suite (k_overlap_walk): the smallest shapes at which the walk with positions can go wrong — a visit's first and last aligned
column on either side of the 64-byte window's edge, an alt-id across it, visits without a column, trimming, the mirrored target interval, and a
read set whose record counts make the offsets come from the scan.  Every stream is walked by overlaps_ref as it is built, and what it was made
for is asserted right here."""
import numpy as np
import overlaps_ref as OR
from editstreams import INS, DEL, MATCH, SUBST, ANCHOR, SKIP, ALT_ID, MAIN_REF, PLAIN, START_PLAIN, START_ES, START_PLAIN_N, REF_LENS, b1, b4, b5, references

F = {k: i for i, k in enumerate(OR.FIELDS)}


def hand_made():
    """name -> stream, every one well formed over references(); the first window holds the stream bytes 5 .. 68"""
    refs = references()
    S = {}

    def put(name, stream, n_rec, **first):
        recs, _ = OR.records_of_read(stream, refs)
        assert len(recs) == n_rec, (name, recs)
        for k, v in first.items():                            # fields of the LAST record
            assert recs[-1][F[k]] == v, (name, k, recs[-1])
        S[name] = stream

    ins, dl, m = b1(INS, 2), b1(DEL), b1(MATCH)
    # the first aligned column of a visit as the last tuple of a window / the first of the next; leading ins and del do not count
    put("first_column_ends_the_window", b5(START_ES, 0) + (ins + dl) * 31 + ins + m + b1(SUBST, 1) + ins, 1, qs=32, ts=31, qe=34, te=33, matches=1, subst=1)
    put("first_column_starts_the_next_window", b5(START_ES, 0) + (ins + dl) * 32 + m + m + dl, 1, qs=32, ts=32, qe=34, te=34, matches=2)
    # the last aligned column at either place; trailing ins and del do not count
    put("last_column_ends_the_window", b5(START_ES, 0, 1) + m * 64 + (ins + dl) * 3, 1, qs=0, qe=64, ts=REF_LENS[0] - 64, te=REF_LENS[0], qlen=67, flags=OR.REV | OR.MAIN)
    put("last_column_starts_the_next_window", b5(START_ES, 0) + m * 65 + (dl + ins) * 3, 1, qs=0, qe=65, ts=0, te=65, qlen=68)
    put("last_column_is_an_anchor_over_the_edge", b5(START_ES, 0) + m * 62 + b4(ANCHOR, 9) + ins * 2, 1, qe=71, te=71, matches=71, anchor_bases=9)
    # an alt-id whose five bytes cross the window's edge at each byte (k of them inside), followed by a match
    for k in range(0, 6):
        put(f"alt_id_{k}_bytes_before_the_edge", b5(START_ES, 0) + m * (64 - k) + b5(ALT_ID, 1, k & 1) + b4(SKIP, 3) + m + m, 2, t=1, qs=64 - k, qe=66 - k,
            ts=REF_LENS[1] - 5 if k & 1 else 3, te=REF_LENS[1] - 3 if k & 1 else 5, flags=k & 1)
    # visits without an aligned column between two alt-ids: insertions only, skips only, deletions only
    put("visits_without_a_column", b5(START_ES, 0) + m + b5(ALT_ID, 1) + ins * 3 + b5(ALT_ID, 2) + b4(SKIP, 5) + b4(SKIP, 2) + b5(ALT_ID, 1) + dl * 3 + b5(ALT_ID, 2, 1) + b4(SKIP, 1) + m,
        2, t=2, qs=4, qe=5, ts=1, te=2, flags=0)
    put("anchor_0_is_no_column", b5(START_ES, 0) + b5(ALT_ID, 1) + b4(SKIP, 3) + b4(ANCHOR, 0) + b1(MAIN_REF) + b4(ANCHOR, 0) + m, 1, t=0, qs=0, qe=1, flags=OR.MAIN)
    put("anchor_0_inside_a_visit", b5(START_ES, 0) + m + b4(ANCHOR, 0) + dl + b4(ANCHOR, 0), 1, qs=0, qe=1, ts=0, te=1)
    # a main-ref while on the main reference closes the visit, and the cursor goes on
    put("main_ref_on_the_main_reference", b5(START_ES, 0) + m * 2 + b1(MAIN_REF) + b1(SUBST, 0) + m + b1(MAIN_REF) + b1(MAIN_REF) + dl + m, 3, qs=4, qe=5, ts=5, te=6, flags=OR.MAIN)
    # the same alternative entered twice: two records, and the orientation of its first appearance holds
    for first in (0, 1):
        put(f"same_alternative_twice_first{first}", b5(START_ES, 0) + b4(ANCHOR, 40) + b5(ALT_ID, 1, first) + b4(SKIP, 7) + b4(ANCHOR, 30) + b1(MAIN_REF) + m + b5(ALT_ID, 1, 1 - first) +
            b4(SKIP, 50) + b4(ANCHOR, 40) + b1(SUBST, 1), 4, t=1, flags=first, qs=71, qe=112, ts=REF_LENS[1] - 91 if first else 50, te=REF_LENS[1] - 50 if first else 91, subst=1, anchor_bases=40)
    # a reversed reference with the last column at tlen: its forward interval starts at 0
    put("reversed_to_the_end", b5(START_ES, 2, 1) + b4(SKIP, 30) + m * 3, 1, t=2, ts=0, te=3, tlen=33, flags=OR.REV | OR.MAIN)
    put("reversed_alternative_anchor_to_the_end", b5(START_ES, 0) + m + b5(ALT_ID, 1, 1) + b4(SKIP, 90) + b4(ANCHOR, 7), 2, t=1, ts=0, te=7, qs=1, qe=8, flags=OR.REV)
    put("forward_to_the_end", b5(START_ES, 2) + b4(SKIP, 30) + m * 3, 1, ts=30, te=33)
    # trimming: leading and trailing runs of ins / del / skip are outside the record, those between columns inside
    put("trimming", b5(START_ES, 0) + ins * 2 + dl * 3 + b4(SKIP, 10) + m + b1(SUBST, 2) + ins + dl + b4(SKIP, 5) + m + ins * 2 + dl * 2 + b4(SKIP, 4), 1, qs=2, qe=6, ts=13, te=22, qlen=8,
        matches=2, subst=1)
    put("columns_only_in_the_second_window", b5(START_ES, 0) + ins * 70 + b5(ALT_ID, 1) + m, 1, t=1, qs=70, qe=71)
    put("visit_over_three_windows", b5(START_ES, 0) + dl + (m + ins) * 80 + b1(SUBST, 0) + dl * 40, 1, qs=0, qe=161, ts=1, te=82, matches=80, subst=1)
    return S


def script_with_records(n, seed):
    """a script read of n >= 1 records: visits on the main reference and on alternatives in turn"""
    rng = np.random.default_rng(seed)
    s = b5(START_ES, 0, seed & 1) + b1(MATCH)
    for i in range(1, n):
        s += (b5(ALT_ID, 3 + int(rng.integers(50)), i & 2) + b4(SKIP, 1 + i % 5) + b1(MATCH) * (1 + i % 3)) if i & 1 else (b1(MAIN_REF) + b1(INS, i % 4) + b1(MATCH) + b1(SUBST, i % 3))
    return s


def read_set():
    """plain reads and script reads with 0, 1 and 66 records in turn: a read's place in the output comes from the scan over all of them"""
    rng = np.random.default_rng(5)
    plain = lambda n: b1(START_PLAIN) + b"".join(b1(PLAIN, int(rng.integers(4))) for _ in range(n))
    none = [b5(START_ES, 0) + b1(INS, 1) * 3, b5(START_ES, 1, 1) + b4(SKIP, 9), b5(START_ES, 2) + b5(ALT_ID, 1) + b1(DEL)]
    out, want = [], []
    for i in range(12):
        for s, n in ((plain(10 + 7 * i), 0), (none[i % 3], 0), (script_with_records(1, i), 1), (script_with_records(66, i), 66), (b1(START_PLAIN_N) + b1(PLAIN, 4), 0)):
            out.append(s)
            want.append(n)
    refs = references()
    assert [len(OR.records_of_read(s, refs)[0]) for s in out] == want
    return out
