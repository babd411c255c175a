"""The content report (cl_report, the `hipreport` stream) restated in numpy from its definition — the yardstick of
tests/test_report_cpu.py, tests/test_gpu_report.py and tests/test_gpu_cli_report.py.  A report is a dict of ints and numpy uint64
arrays with the field names of cl_report, plus n50 / n90 where all read lengths are known.  The quality VALUES come from
tests/qual_values_ref.py (the decoder's recurrence, checked there); report_loops() states every field again in plain Python loops, for
small reads, and tests/test_report_cpu.py holds the two against each other."""
import struct
import numpy as np
import qual_values_ref as V

U64_MAX = (1 << 64) - 1
FIELDS = ("reads", "bases", "base_count", "len_min", "len_max", "len_hist", "len_bases", "has_qual", "q_reads", "q_symbols", "mean_q_hist", "q_joint")


def empty():
    return dict(reads=0, bases=0, base_count=np.zeros(5, np.uint64), len_min=U64_MAX, len_max=0, len_hist=np.zeros(33, np.uint64), len_bases=np.zeros(33, np.uint64),
                has_qual=0, q_reads=0, q_symbols=0, mean_q_hist=np.zeros(96, np.uint64), q_joint=np.zeros((96, 96), np.uint64))


def nxx(lengths, pct):
    """sort descending; the length at which the running sum first reaches pct % of the bases (0 without bases)"""
    ls = sorted((int(x) for x in lengths), reverse=True)
    total, run = sum(ls), 0
    for x in ls:
        run += x
        if x and run * 100 >= total * pct:
            return x
    return 0


def _phred(ascii_bytes):
    p = np.asarray(ascii_bytes, np.int64) - 33
    return np.where((p < 0) | (p > 95), 0, p)


def report(codes, quals_ascii=None, mode=None, T=None, D=None):
    """codes: per read its base codes (0..3, 4 and above = N); quals_ascii: per read its INPUT quality bytes (None: no quality part);
    mode: the quality mode's name ("none": no quality part)"""
    r = empty()
    lens = np.array([len(c) for c in codes], np.int64)
    r["reads"], r["bases"] = len(codes), int(lens.sum())
    if len(codes):
        allc = np.concatenate([np.asarray(c, np.uint8) & 7 for c in codes]) if r["bases"] else np.zeros(0, np.uint8)
        r["base_count"] = np.bincount(np.minimum(allc, 4), minlength=5).astype(np.uint64)
        r["len_min"], r["len_max"] = int(lens.min()), int(lens.max())
        bins = np.array([int(x).bit_length() for x in lens], np.int64)
        r["len_hist"] = np.bincount(bins, minlength=33).astype(np.uint64)
        r["len_bases"] = np.bincount(bins, weights=lens.astype(np.float64), minlength=33).astype(np.uint64)
    r["n50"], r["n90"] = nxx(lens, 50), nxx(lens, 90)
    if quals_ascii is not None and mode not in (None, "none"):
        r["has_qual"] = 1
        r["q_reads"] = len(quals_ascii)
        for q in quals_ascii:
            p = _phred(q)
            out = np.minimum(V.values_int(mode, p, T, D).astype(np.int64), 95)
            np.add.at(r["q_joint"], (p, out), np.uint64(1))
            r["q_symbols"] += len(p)
            if len(p):
                r["mean_q_hist"][int(p.sum()) // len(p)] += np.uint64(1)
    return r


def report_loops(codes, quals_ascii=None, mode=None, T=None, D=None):
    """the same in plain Python loops, the values from the decoder's double recurrence (qual_values_ref.values_double)"""
    r = empty()
    for c in codes:
        n = len(c)
        r["reads"] += 1; r["bases"] += n
        for x in c:
            r["base_count"][min(int(x) & 7, 4)] += np.uint64(1)
        r["len_min"], r["len_max"] = min(r["len_min"], n), max(r["len_max"], n)
        b = 0
        while (n >> b) > 0:
            b += 1
        r["len_hist"][b] += np.uint64(1); r["len_bases"][b] += np.uint64(n)
    r["n50"], r["n90"] = nxx([len(c) for c in codes], 50), nxx([len(c) for c in codes], 90)
    if quals_ascii is not None and mode not in (None, "none"):
        r["has_qual"] = 1
        for q in quals_ascii:
            p = [int(x) - 33 if 0 <= int(x) - 33 <= 95 else 0 for x in q]
            out = V.values_double(mode, np.array(p, np.int64), T, D)
            for a, b in zip(p, out):
                r["q_joint"][a][min(int(b), 95)] += np.uint64(1)
            r["q_reads"] += 1; r["q_symbols"] += len(p)
            if p:
                r["mean_q_hist"][sum(p) // len(p)] += np.uint64(1)
    return r


def out_marginal(r):
    return np.asarray(r["q_joint"], np.uint64).sum(axis=0)


def in_marginal(r):
    return np.asarray(r["q_joint"], np.uint64).sum(axis=1)


def values_report(values_ascii):
    """what cl_report_values_host gives for DECODED quality lines: q_reads, q_symbols and row 0 of q_joint = the OUT marginal"""
    r = empty()
    r["has_qual"] = 1
    for v in values_ascii:
        o = np.minimum((np.asarray(v, np.int64) - 33) & 0xff, 95)
        r["q_joint"][0] += np.bincount(o, minlength=96).astype(np.uint64)
        r["q_reads"] += 1; r["q_symbols"] += len(o)
    return r


def add(a, b):
    r = empty()
    for k in FIELDS:
        if k == "len_min":
            r[k] = min(a[k], b[k])
        elif k == "len_max":
            r[k] = max(a[k], b[k])
        elif k == "has_qual":
            r[k] = a[k] | b[k]
        else:
            r[k] = a[k] + b[k]
    return r


def same(a, b, fields=FIELDS):
    """the first field in which two reports differ, or None"""
    for k in fields:
        if not np.array_equal(np.asarray(a[k], np.uint64), np.asarray(b[k], np.uint64)):
            return k
    return None


def loss(r):
    """share unchanged, MAE, RMSE, max |delta| of q_joint"""
    J = np.asarray(r["q_joint"], np.float64)
    n = J.sum()
    if not n:
        return dict(unchanged=1.0, mae=0.0, rmse=0.0, max_abs=0)
    d = np.abs(np.arange(96)[:, None] - np.arange(96)[None, :])
    return dict(unchanged=float(np.trace(J) / n), mae=float((J * d).sum() / n), rmse=float(np.sqrt((J * d * d).sum() / n)), max_abs=int(d[J > 0].max()))


# ---- the `hipreport` stream ------------------------------------------------------------------------------------------------------------------
def pack_hipreport(r, version=1):
    """u32 version, u32 flags (bit 0: quality part), reads, bases, base_count[5], len_min, len_max, n50, n90, len_hist[33], len_bases[33]; with
    bit 0: q_reads, q_symbols, mean_q_hist[96], u32 n_cells, the non-zero cells (u8 in, u8 out, u64 count) ascending by (in, out)"""
    b = struct.pack("<II", version, 1 if r["has_qual"] else 0)
    b += struct.pack("<2Q5Q4Q", r["reads"], r["bases"], *[int(x) for x in r["base_count"]], r["len_min"], r["len_max"], r["n50"], r["n90"])
    b += struct.pack("<33Q33Q", *[int(x) for x in r["len_hist"]], *[int(x) for x in r["len_bases"]])
    if r["has_qual"]:
        b += struct.pack("<2Q96Q", r["q_reads"], r["q_symbols"], *[int(x) for x in r["mean_q_hist"]])
        J = np.asarray(r["q_joint"], np.uint64)
        cells = [(i, j, int(J[i, j])) for i in range(96) for j in range(96) if J[i, j]]
        b += struct.pack("<I", len(cells))
        for c in cells:
            b += struct.pack("<BBQ", *c)
    return b


def unpack_hipreport(b):
    r = empty()
    version, flags = struct.unpack_from("<II", b, 0)
    v = struct.unpack_from("<77Q", b, 8)
    r["reads"], r["bases"] = v[0], v[1]
    r["base_count"] = np.array(v[2:7], np.uint64)
    r["len_min"], r["len_max"], r["n50"], r["n90"] = v[7:11]
    r["len_hist"], r["len_bases"] = np.array(v[11:44], np.uint64), np.array(v[44:77], np.uint64)
    at = 8 + 77 * 8
    if flags & 1:
        q = struct.unpack_from("<98Q", b, at); at += 98 * 8
        r["has_qual"], r["q_reads"], r["q_symbols"], r["mean_q_hist"] = 1, q[0], q[1], np.array(q[2:], np.uint64)
        (n,) = struct.unpack_from("<I", b, at); at += 4
        for _ in range(n):
            i, j, c = struct.unpack_from("<BBQ", b, at); at += 10
            r["q_joint"][i, j] = c
    assert at == len(b) and version == 1
    return r
