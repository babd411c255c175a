"""Constructed operation words for the coded CIGARs, shared by the CPU suite (host twin, decoder, sanitizer program) and the GPU suite
(cl_cigars_pack).  All run with part_ops = 16 and seg_ops = 256 where not said otherwise, so that small inputs cross every boundary: a part, a group
of 64 parts, a segment.  What a case was made for is asserted right here, with the judge (tests/cigarcoder_ref.py)."""
import numpy as np
import cigarcoder_ref as CC

PART, SEG = 16, 256
I, D, EQ, X = 1, 2, 7, 8


def words_of(ops, lens):
    return (np.asarray(lens, np.uint32) << 4 | np.asarray(ops, np.uint32)).astype(np.uint32)


def ont_like(n, seed=5):
    """an ONT-like draw: = runs geometric around 13 between single X / I / D, now and then a longer gap or two edits in a row"""
    rng = np.random.default_rng(seed)
    is_eq = np.arange(n) % 2 == 0
    is_eq ^= rng.random(n) < 0.1                                             # two edits, or two = runs, in a row
    ops = np.where(is_eq, EQ, rng.choice([X, I, D], n, p=[0.45, 0.25, 0.30]))
    lens = np.where(is_eq, rng.geometric(1 / 13, n), np.where(rng.random(n) < 0.85, 1, rng.geometric(0.4, n)))
    lens = np.where(rng.random(n) < 0.002, rng.integers(256, 5000, n), lens)     # a long anchor run now and then
    return words_of(ops, lens)


def mixed(n, seed=1):
    rng = np.random.default_rng(seed)
    return words_of(rng.choice([I, D, EQ, X], n), rng.choice([1, 1, 2, 3, 40, 254, 255, 256, 300], n))


def cases():
    """name -> (words, part_ops, seg_ops)"""
    S = {}
    for n in (0, 1, 15, 16, 17, 255, 256, 257):
        S["n%d" % n] = (mixed(n, n), PART, SEG)
    for n in (1023, 1024, 1025):                                              # a group of 64 parts and one more: one segment
        S["n%d_one_segment" % n] = (mixed(n, n), PART, 0)
        S["n%d" % n] = (mixed(n, n), PART, SEG)
    # the escape boundary; escapes on both sides of a part boundary (15 | 16) and of a segment boundary (255 | 256)
    S["escape_boundary"] = (words_of([EQ, D, EQ, I, X], [255, 256, 257, (1 << 28) - 1, 254]), PART, SEG)
    w = mixed(300, 3); w = (w & 0xf) | (np.uint32(2) << 4)
    for at in (15, 16, 255, 256):
        w[at] = (w[at] & 0xf) | (np.uint32(1000 + at) << 4)
    S["escapes_at_the_boundaries"] = (w, PART, SEG)
    counts, escapes, _ = CC.segment_pieces(list(w[:256]), PART)
    assert escapes == [1015, 1016, 1255] and CC.segment_pieces(list(w[256:]), PART)[1] == [1256]
    # one symbol only: freq = tot in every context in use, the parts are their 8 end bytes
    S["one_symbol"] = (words_of([EQ] * 100, [5] * 100), PART, SEG)
    assert all(len(p) == 8 for p in CC.segment_pieces(list(S["one_symbol"][0]), PART)[2])
    # all in one length bin but one operation: the contended bin
    w = words_of([X] * 2000, [1] * 2000); w[777] = 7 << 4 | EQ
    S["one_bin_but_one"] = (w, PART, 0)
    # all four ops after each of the five contexts
    w = mixed(400, 11)
    counts = [0] * CC.BINS
    for s0 in range(0, 400, SEG):
        counts = [a + b for a, b in zip(counts, CC.segment_pieces(list(w[s0:s0 + SEG]), PART)[0])]
    assert min(counts[:20]) > 0
    S["every_op_after_every_context"] = (w, PART, SEG)
    S["ont_like_5000"] = (ont_like(5000), PART, SEG)
    assert (S["ont_like_5000"][0] >> 4 > 255).any()
    return S


def bad_cases():
    """name -> (words, the index of the first word that is no operation)"""
    B = {}
    for what, bad in (("op0", 3 << 4 | 0), ("op9", 3 << 4 | 9), ("len0", EQ)):
        for where, at in (("first", 0), ("last", 99), ("first_of_a_part", 16)):
            w = mixed(100, 2); w[at] = bad
            B["%s_%s" % (what, where)] = (w, at)
    w = mixed(100, 2); w[40] = 9; w[16] = 0
    B["two_bad"] = (w, 16)
    return B
