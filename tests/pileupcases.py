"""Constructed genomes and tuple streams for the pileup, shared by tests/test_pileup_cpu.py, tests/test_gpu_pileup.py and the sanitized
host program: the smallest shapes at which the walk, the fold and the site search can go wrong.

HAND: the hand-made streams of tests/editstreams.py, unchanged, with their 69 references taken as 69 one-piece sequences (pieces of 80 000 bases
every 79 900): the window's edge, runs across it, both orientations, 64 alternatives, anchors of 0, 1, 63, 64, 65 and 70 000 bases.
NINE: the nine sequences of tests/mappingcases.py in pieces of 100 every 70 — 20 pieces, one-base pieces and an empty sequence among them —
followed by three reference READS (ids 20, 21, 22), and constructed streams over them, in named groups."""
import numpy as np
import editstreams as ES
import mappingcases as MC
import pileup_ref as PR
from editstreams import b1, b4, b5, INS, DEL, MATCH, SUBST, ANCHOR, SKIP, ALT_ID, MAIN_REF, START_ES

THRESHOLDS = [PR.DEFAULTS, (0, 0, 0), (1, 1, 333), (1, 1, 334), (1, 1, 1000), (13, 3, 230), (13, 3, 231), (5, 4, 0)]
READ_COUNTS = [0, 1, 4, 5, 1025]


class Case:
    def __init__(self, seqs, read_len, overlap, extra_refs, streams):
        self.seqs, self.read_len, self.overlap = seqs, read_len, overlap
        self.refs = PR.cut(seqs, read_len, overlap) + list(extra_refs)       # the pieces are the first references
        self.seq_len = [len(s) for s in seqs]
        self.streams = list(streams)

    def judged(self, streams=None):
        T = PR.Table(self.seqs, self.read_len, self.overlap)
        T.add(self.streams if streams is None else streams, self.refs)
        return T.fold()


def hand():
    S = ES.hand_made()
    return Case(ES.references(), 80_000, 100, [], S.values()), list(S)


# ---- the nine sequences -------------------------------------------------------------------------------------------------------------------
P = PR.pieces(**MC.NINE)                                      # (sequence, start, length) of pieces 0 .. 19
N_POS = sum(MC.NINE["seq_len"])
READ_IDS = (20, 21, 22)


def nine_seqs(seed=31):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, n).astype(np.uint8) for n in MC.NINE["seq_len"]]


def nine_extra(seed=32):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, n).astype(np.uint8) for n in (50, 60, 200)]


def one(piece, cursor, tuples, rev=0):
    """a read that goes to `cursor` of a piece and says `tuples` there"""
    return b5(START_ES, piece, rev) + (b4(SKIP, cursor) if cursor else b"") + tuples


def column(piece, cursor, match=0, sub=(0, 0, 0), dele=0, ins=0):
    """single-tuple reads that give the position at `cursor` of a piece (taken forward) these counts; an insertion run is booked left of it"""
    out = [one(piece, cursor, b1(MATCH))] * match + [one(piece, cursor, b1(DEL))] * dele + [one(piece, cursor + 1, b1(INS, 2))] * ins
    for v, n in enumerate(sub):
        out += [one(piece, cursor, b1(SUBST, v))] * n
    return out


def groups():
    """name -> streams over the nine sequences"""
    assert len(P) == 20 and P[13] == (6, 0, 1) and P[9] == (4, 140, 1) and P[19] == (8, 0, 69) and P[6] == (3, 70, 30) and N_POS == 1147
    G = {}
    # two reads reach positions 80 .. 94 of sequence 0 through pieces 0 and 1; the second says a substitution, a deletion and an insertion there
    G["same_positions_through_two_pieces"] = [one(0, 80, b4(ANCHOR, 15) + b1(MATCH)), one(1, 10, b4(ANCHOR, 5) + b1(SUBST, 1) + b1(DEL) + b1(INS, 0) + b4(ANCHOR, 8), 0),
                                              one(1, 75, b4(ANCHOR, 15), 1)]
    G["anchors_at_both_ends_of_the_table"] = [one(0, 0, b4(ANCHOR, 100)), one(0, 90, b4(ANCHOR, 10), 1), one(19, 9, b4(ANCHOR, 60)), one(19, 0, b4(ANCHOR, 10), 1), one(19, 0, b4(ANCHOR, 69), 1),
                                              one(19, 68, b1(SUBST, 0))]
    G["one_base_pieces"] = [one(13, 0, b4(ANCHOR, 1), 1), one(13, 0, b4(ANCHOR, 1)), one(9, 0, b4(ANCHOR, 1), 1), one(9, 0, b1(SUBST, 2), 1), one(13, 0, b1(DEL)), one(13, 0, b4(ANCHOR, 0), 1)]
    G["insertion_runs_without_a_position"] = [one(5, 0, b1(INS, 1) * 3 + b1(MATCH)), one(6, 0, b4(ANCHOR, 30) + b1(INS, 0) * 2, 1), one(13, 5, b1(INS, 3)), one(13, 1, b1(INS, 3), 1)]
    G["insertion_runs_at_the_last_base"] = [one(6, 0, b4(ANCHOR, 30) + b1(INS, 2)), one(6, 0, b4(ANCHOR, 29) + b1(INS, 2), 1), one(6, 0, b1(INS, 2) * 5, 1), one(13, 1, b1(INS, 0)), one(13, 0, b1(INS, 0), 1)]
    G["insertion_run_over_the_windows_edge"] = [one(14, 0, b1(MATCH) * (64 - k) + b1(INS, 1) * 4 + b1(MATCH)) for k in (1, 2, 3)] + [one(14, 0, b1(MATCH) * 64 + b1(INS, 1) * 130 + b1(MATCH), 1)]
    G["insertion_run_cut_by_a_change_of_reference"] = [
        one(14, 0, b1(MATCH) * 3 + b1(INS, 0) * 2 + b5(ALT_ID, 15, 0) + b1(INS, 0) * 2 + b1(MATCH)),                         # two runs, the second at cursor 0: no position
        one(14, 0, b1(MATCH) * 3 + b1(INS, 0) * 2 + b5(ALT_ID, 15, 1) + b1(INS, 0) * 2 + b1(MATCH)),                         # ... reversed: the alternative's last base
        one(14, 0, b1(MATCH) * 3 + b5(ALT_ID, 16, 0) + b4(SKIP, 4) + b1(INS, 3) + b1(MAIN_REF) + b1(INS, 3) + b1(MATCH)),  # cut by a main-ref
        one(14, 0, b1(MATCH) * 56 + b1(INS, 1) + b5(ALT_ID, 15, 0) + b4(SKIP, 2) + b1(INS, 1) + b1(MATCH)),                # the alt-id ends the window, the run after it opens the next
        one(14, 0, b1(MATCH) * 58 + b1(INS, 1) + b5(ALT_ID, 15, 0) + b1(INS, 1) * 3)]                                         # an ins is the window's first tuple behind an alt-id
    G["every_substitution"] = [b5(START_ES, 16, rev) + b1(SUBST, v) * 100 for rev in (0, 1) for v in (0, 1, 2)]
    G["reads_on_reads"] = [b5(START_ES, 20) + b1(MATCH) * 5 + b1(INS, 1) + b5(ALT_ID, 21, 1) + b4(ANCHOR, 10) + b1(SUBST, 0) + b1(DEL),
                           b5(START_ES, 22, 1) + b4(ANCHOR, 200)]
    G["a_read_and_a_piece_in_turn"] = [b5(START_ES, 21) + b1(MATCH) * 2 + b5(ALT_ID, 2, 1) + b4(SKIP, 3) + b1(MATCH) + b1(SUBST, 0) + b1(INS, 0) + b1(MAIN_REF) + b1(INS, 0) + b1(DEL) +
                                       b5(ALT_ID, 2, 0) + b4(ANCHOR, 7),
                                       b5(START_ES, 2) + b4(ANCHOR, 20) + b5(ALT_ID, 22) + b1(INS, 1) * 3 + b4(ANCHOR, 9) + b1(MAIN_REF) + b1(MATCH)]
    G["contention_1025_reads_on_one_position"] = [one(4, 7, b1(SUBST, 1) + b1(DEL) + b1(INS, 2) + b4(ANCHOR, 3))] * 1025
    T = []                                                     # thresholds, on piece 10 (sequence 5): default 4 / 3 / 250
    T += column(10, 10, match=2, sub=(2, 0, 0))                # alt = min_alt - 1
    T += column(10, 20, match=1, sub=(0, 3, 0))                # alt = min_alt
    T += column(10, 30, match=9, sub=(0, 0, 3))                # alt * 1000 = min_permille * depth
    T += column(10, 40, match=10, sub=(3, 0, 0))               # ... and below it: 3000 < 250 * 13 (231 * 13 = 3003, 230 * 13 = 2990)
    T += column(10, 50, match=1, sub=(3, 3, 0), dele=3, ins=3)      # the tie of all kinds: the lowest base that is not the reference's
    T += column(10, 60, match=1, dele=3, ins=3)                # the tie of del and ins
    T += column(10, 65, match=2, sub=(0, 0, 1))                # 1000 / 3: 333 passes, 334 does not
    T += column(10, 70, ins=5)                                 # an insertion run where nothing aligns: depth 0
    T += column(10, 75, dele=4)                                # every column a deletion
    G["thresholds"] = T
    return G


def nine(streams):
    return Case(nine_seqs(), MC.NINE["read_len"], MC.NINE["overlap"], nine_extra(), streams)


def everything():
    """one read set of all groups, three reads of the contention's"""
    return [s for name, g in groups().items() for s in (g[:3] if name.startswith("contention") else g)]
