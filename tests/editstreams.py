"""Hand-made tuple streams for the edit-operation profile, shared by the CPU suite (host form, sanitizer program) and the GPU
suite (k_edit_profile): the smallest shapes at which the walk can go wrong — the 64-byte window's edge, runs across it, the values at which a
histogram bin changes, the alternative table full.  References: 70 001, 97 and 33 bases as in tests/test_gpu_expand.py, then 66 short ones
(ids 3..68) for the alternatives.  Every well-formed stream here is checked by edits_ref (it raises on a position outside a reference)."""
import numpy as np

INS, DEL, MATCH, SUBST, ANCHOR, SKIP, ALT_ID, MAIN_REF, PLAIN, START_PLAIN, START_ES, START_PLAIN_N = range(12)
REF_LENS = (70_001, 97, 33) + tuple(24 + (i % 17) for i in range(66))
HEAD = 5                                                    # the start-es tuple: the first window begins behind it


def b1(t, lo=0): return bytes([(t << 4) | lo])
def b4(t, v): return bytes([(t << 4) | (v >> 24)]) + (v & 0xffffff).to_bytes(3, "big")
def b5(t, rid, rev=0): return bytes([(t << 4) | (1 if rev else 0)]) + rid.to_bytes(4, "big")


def references(seed=12):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, n).astype(np.uint8) for n in REF_LENS]


def expand_family(rng):
    """the window-edge family of tests/test_gpu_expand.py, rebuilt here tuple for tuple (the CPU suite imports nothing of the GPU suites): unit runs of 55..65, then
    an anchor and an alt-id that cross the window's edge at each of their bytes; anchors at the word boundaries; the same alternative twice; 100 000 units"""
    S = {}
    unit = lambda: [b1(INS, int(rng.integers(4))), b1(DEL), b1(MATCH), b1(SUBST, int(rng.integers(3)))][int(rng.integers(4))]
    for run in range(55, 66):
        S[f"edge_run{run}"] = b5(START_ES, 0, run & 1) + b"".join(unit() for _ in range(run)) + b4(ANCHOR, 37) + b5(ALT_ID, 1 + (run & 1), run & 2) + b4(SKIP, 3) + b4(ANCHOR, 20) + \
            b1(MAIN_REF) + b"".join(unit() for _ in range(70 - run)) + b4(ANCHOR, 5)
    for rev in (0, 1):
        for a in (1, 31, 32, 33, 63, 64, 65, 4097, 70_000):
            for p in (0, 1, 31, 32, 33):
                if p + a <= REF_LENS[0]:
                    S[f"anchor{a}_at{p}_rev{rev}"] = b5(START_ES, 0, rev) + (b4(SKIP, p) if p else b"") + b4(ANCHOR, a)
    for first in (0, 1):      # the same alternative twice, the second time with the other orientation nibble: the first one holds, and it is ONE alternative
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


def hand_made(seed=12):
    """name -> stream, every one well formed over references()"""
    rng = np.random.default_rng(seed)
    S = expand_family(rng)
    ins = lambda n: b"".join(b1(INS, int(rng.integers(4))) for _ in range(n))
    pad = lambda n: b1(MATCH) * n                             # n one-byte tuples on reference 0 in front of what is placed
    for L in (2, 3, 4):                                       # a run of L with `first` of its tuples in the first window
        for first in range(1, L):
            S[f"ins_run{L}_split{first}"] = b5(START_ES, 0) + pad(64 - first) + ins(L) + b1(MATCH)
            S[f"del_run{L}_split{first}"] = b5(START_ES, 0, 1) + pad(64 - first) + b1(DEL) * L + b1(MATCH)
            S[f"ins_run{L}_split{first}_ends_stream"] = b5(START_ES, 0) + pad(64 - first) + ins(L)
    for L in (15, 16, 17, 200):
        S[f"ins_run{L}"] = b5(START_ES, 0) + b1(MATCH) + ins(L) + b1(MATCH)
        S[f"del_run{L}"] = b5(START_ES, 0) + b1(MATCH) + b1(DEL) * L + b1(SUBST, 1)
        S[f"ins_run{L}_from_the_start"] = b5(START_ES, 0) + ins(L)
    S["ins_run_then_del_run"] = b5(START_ES, 0) + b1(MATCH) + ins(3) + b1(DEL) * 2 + b1(MATCH)
    S["ins_run_to_the_edge_then_del_run"] = b5(START_ES, 0) + pad(61) + ins(3) + b1(DEL) * 3 + ins(1)
    S["del_run_over_the_edge_then_ins_run"] = b5(START_ES, 0) + pad(62) + b1(DEL) * 4 + ins(70) + b1(DEL)
    S["alt_id_ends_the_window_skip_starts_the_next"] = b5(START_ES, 0) + pad(59) + b5(ALT_ID, 1, 1) + b4(SKIP, 11) + b4(ANCHOR, 10) + b1(MAIN_REF) + b1(MATCH)
    S["skip_after_main_ref"] = b5(START_ES, 0) + b1(MATCH) + b5(ALT_ID, 1) + b4(SKIP, 3) + b1(MATCH) + b1(MAIN_REF) + b4(SKIP, 4) + b1(MATCH)
    S["skip_first"] = b5(START_ES, 0) + b4(SKIP, 5) + b1(MATCH)
    S["alt_id_without_skip"] = b5(START_ES, 0) + b1(MATCH) + b5(ALT_ID, 2) + b1(MATCH) + b4(SKIP, 6) + b1(DEL)
    for a in (1, 2, 31, 32, 63, 64, 4095, 4096, 70_000):      # 1, 2^k - 1 and 2^k for k = 1, 5, 6, 12: the bins' edges
        S[f"anchor_len{a}"] = b5(START_ES, 0) + b1(MATCH) + b4(ANCHOR, a) + b1(INS, 1)
        S[f"skip_len{a}"] = b5(START_ES, 0, 1) + b4(SKIP, a) + b1(MATCH)
    S["anchor_len0"] = b5(START_ES, 0) + b4(ANCHOR, 0) + b4(SKIP, 0) + b1(MATCH)
    S["reversed_main_and_alternative"] = b5(START_ES, 1, 1) + b1(MATCH) * 5 + b1(SUBST, 0) + b1(DEL) + b5(ALT_ID, 2, 1) + b4(SKIP, 4) + b1(MATCH) * 3 + b1(SUBST, 2) + b1(DEL) + b1(MAIN_REF) + b1(MATCH)
    S["alternatives_64"] = b5(START_ES, 0) + b1(MATCH) + b"".join(b5(ALT_ID, 2 + i, i & 1) + b4(SKIP, 1) + b1(MATCH) + b1(SUBST, i % 3) for i in range(1, 65)) + b1(MAIN_REF) + b1(MATCH)
    S["alternatives_64_each_twice"] = b5(START_ES, 0) + b"".join(b5(ALT_ID, 2 + i, 0) + b1(MATCH) for i in range(1, 65)) + b"".join(b5(ALT_ID, 2 + i, 1) + b1(DEL) for i in range(64, 0, -1))
    S["identity_0"] = b5(START_ES, 0) + b1(SUBST, 0) + b1(SUBST, 1) + b1(SUBST, 2) + b1(INS, 0) + b1(INS, 3) + b1(DEL)
    S["identity_100"] = b5(START_ES, 0) + b4(ANCHOR, 50) + b1(MATCH) * 3
    S["identity_99"] = b5(START_ES, 0) + b4(ANCHOR, 99) + b1(SUBST, 1)
    S["skips_only"] = b5(START_ES, 0) + b4(SKIP, 5) + b4(SKIP, 7)
    S["start_only"] = b5(START_ES, 2, 1)
    S["plain"] = b1(START_PLAIN) + b"".join(b1(PLAIN, int(rng.integers(4))) for _ in range(200))
    S["plain_with_n"] = b1(START_PLAIN_N) + b"".join(b1(PLAIN, int(rng.integers(5))) for _ in range(77)) + b1(PLAIN, 4)
    S["plain_empty"] = b1(START_PLAIN)
    S["plain_one"] = b1(START_PLAIN_N) + b1(PLAIN, 4)
    return S


def malformed_host():
    """name -> (stream, what it runs into): for the host form alone — an id, a position or a tuple out of range is never given to the device"""
    M = {
        "truncated_anchor": (b5(START_ES, 0) + b1(MATCH) + b4(ANCHOR, 9)[:3], "tuple crosses the end of the stream"),
        "truncated_skip_one_byte": (b5(START_ES, 0) + b4(SKIP, 9)[:1], "tuple crosses the end of the stream"),
        "truncated_alt_id": (b5(START_ES, 0) + b1(MATCH) * 62 + b5(ALT_ID, 1)[:4], "tuple crosses the end of the stream"),
        "truncated_start": (b5(START_ES, 0)[:4], "tuple crosses the end of the stream"),
        "main_id_out_of_range": (b5(START_ES, len(REF_LENS)) + b1(INS, 0), "reference id outside the reference arena"),
        "alt_id_out_of_range": (b5(START_ES, 0) + b5(ALT_ID, 0xffffffff) + b1(INS, 0), "reference id outside the reference arena"),
        "match_on_the_guard": (b5(START_ES, 2) + b4(SKIP, 33) + b1(MATCH), "position outside the reference read"),
        "del_on_the_guard": (b5(START_ES, 2, 1) + b4(ANCHOR, 33) + b1(DEL), "position outside the reference read"),
        "subst_on_the_guard": (b5(START_ES, 1) + b5(ALT_ID, 2) + b4(SKIP, 40) + b1(SUBST, 0), "position outside the reference read"),
        "anchor_past_the_end": (b5(START_ES, 2) + b1(MATCH) + b4(ANCHOR, 33), "position outside the reference read"),
        "alternative_65": (b5(START_ES, 0) + b"".join(b5(ALT_ID, 2 + i) for i in range(1, 66)), "more than 64 alternative references"),
        "first_tuple_match": (b1(MATCH) + b1(MATCH), "first tuple is no start tuple"),
        "first_tuple_type_13": (bytes([0xd0]) + b1(MATCH), "first tuple is no start tuple"),
        "empty": (b"", "empty stream"),
    }
    return M


def malformed_device():
    """name -> (stream, what it runs into): malformed, yet inside every buffer whether or not a check were missing"""
    return {
        "type_12_inside_a_script": (b5(START_ES, 0) + b1(MATCH) * 3 + bytes([0xc0]) + b1(MATCH), "tuple type not allowed inside an edit script"),
        "subst_value_3": (b5(START_ES, 0) + b1(MATCH) + b1(SUBST, 3), "base value out of range"),
        "ins_value_7": (b5(START_ES, 0, 1) + b1(MATCH) * 70 + b1(INS, 7), "base value out of range"),
    }
