"""Constructed geometries and overlap records for the lift of the read-to-genome mappings, shared by tests/test_mappings_cpu.py,
tests/test_gpu_mappings.py and the sanitized host program: the smallest shapes at which the lift can go wrong."""
import numpy as np
import mappings_ref as MR

# nine sequences, pieces of 100 bases every 70: 250 -> 4 pieces (the last 40 long); NO base -> no piece, between two others; 70 -> one piece (exactly
# a step); 100 -> two pieces (the last 30 long: exactly the overlap); 141 -> three pieces, the last ONE base long (shorter than the overlap);
# 171 -> three; 1 -> one piece of one base; 345 -> five; 69 -> one piece
NINE = dict(seq_len=[250, 0, 70, 100, 141, 171, 1, 345, 69], read_len=100, overlap=30)
ONE = dict(seq_len=[1000], read_len=300, overlap=50)            # one sequence: 4 pieces, the last 250 long
GEOMETRIES = {"nine": NINE, "one": ONE}
SIZES = [0, 1, 64, 65, 257, 1025]
MODES = ["none_dropped", "all_dropped", "alternating"]


def n_pseudo(geo):
    return len(MR.pieces(**geo))


def record(rng, q, t, tlen):
    """a record on a target of tlen bases (tlen >= 1) with everything else drawn: both strands, main reference and alternatives"""
    ts = int(rng.integers(0, tlen))
    te = int(rng.integers(ts + 1, tlen + 1))
    m = int(rng.integers(1, te - ts + 1))
    sb = int(rng.integers(0, te - ts - m + 1))
    qs = int(rng.integers(0, 50))
    qe = qs + m + sb + int(rng.integers(0, 9))
    return (q, t, qe + int(rng.integers(0, 7)), tlen, qs, qe, ts, te, m, sb, int(rng.integers(0, m + 1)), int(rng.integers(0, 4)))


def records(geo, n, mode, seed=1):
    """n records in `mode`; the kept ones walk the first and the last piece of every sequence first (t = n_pseudo - 1 among them), then every
    piece in turn; the dropped ones name reads: t = n_pseudo first, then ids behind it"""
    rng = np.random.default_rng(seed + n)
    P = MR.pieces(**geo)
    first_last = []
    for s in range(len(geo["seq_len"])):
        mine = [i for i, p in enumerate(P) if p[0] == s]
        if mine:
            first_last += [mine[0], mine[-1]]
    order = first_last[::-1] + list(range(len(P)))
    out, kept, dropped = [], 0, 0
    for i in range(n):
        keep = mode == "none_dropped" or (mode == "alternating" and i % 2 == 1)
        if keep:
            t = order[kept % len(order)]; kept += 1
            out.append(record(rng, 7 + i // 3, t, P[t][2]))
        else:
            t = len(P) + (0 if dropped == 0 else int(rng.integers(0, 1000))); dropped += 1
            out.append(record(rng, 7 + i // 3, t, int(rng.integers(1, 5000))))
    return np.array(out, np.uint32).reshape(-1, 12)


def refused(geo=NINE):
    """name -> (records, the first refused record, its code): each a record that cannot be lifted among good ones, a second bad one behind it"""
    P = MR.pieces(**geo)
    base = records(geo, 200, "alternating", seed=5)
    kept = [i for i in range(len(base)) if base[i, 1] < len(P)]
    last_of_seq0 = max(i for i, p in enumerate(P) if p[0] == 0)              # a piece that is not its sequence's first, and its last
    out = {}
    for name, code in (("tlen", MR.TLEN), ("position", MR.POS), ("end", MR.END)):
        r = base.copy()
        for at in (kept[37], kept[60]):
            r[at, 1] = last_of_seq0; r[at, 3] = P[last_of_seq0][2]; r[at, 6] = 0; r[at, 7] = 1
            if code == MR.TLEN:
                r[at, 3] += 1
            elif code == MR.POS:
                r[at, 7] = 0xffffffff
            else:
                r[at, 7] = r[at, 3] + 1
        out[name] = (r, kept[37], code)
    return out
