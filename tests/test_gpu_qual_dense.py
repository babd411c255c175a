"""GPU suite for the dense context ids of the per-base quality family and for the sort's last digit.

The quality coder numbers a context by the values its fields can take (a history field: a symbol, or "no such position"), sorts by that
id and lets the model kernels find their own runs in the sorted keys.  Any one-to-one numbering gives the reference's bytes, so
everything here is compared with the oracle: read sets in which EVERY history field is missing somewhere (reads of 1 .. 8 bases: the
binary modes look 6 positions back), qualities over all bins, and one encode split over two calls (the models persist).  The sort is
checked on keys with non-zero bits above `end_bit`: they must come out ordered on the requested bits alone, and stable."""
import numpy as np
import pytest
import torch
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

PER_BASE_MODES = [0, 1, 2, 3, 4, 5, 6]


def short_and_long_reads(seed, quals_of):
    from colord_amd.fastq import ReadSet
    rng = np.random.default_rng(seed)
    lens = []
    for rep in range(40):                                   # many reads of every length 1 .. 8, mixed with long ones
        lens += list(rng.permutation(np.arange(1, 9)))
        lens.append(int(rng.integers(9, 400)))
        if rep % 8 == 0:
            lens.append(int(rng.integers(20_000, 70_000)))
    lens = np.asarray(lens, np.int64)
    n = int(lens.sum())
    bases = rng.integers(0, 4, n, dtype=np.uint8)
    quals = (33 + quals_of(rng, n)).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return ReadSet(bases, off, quals, [b"r%d" % i for i in range(len(lens))], [False] * len(lens), True)


def gpu_encode(ctx, rs, mode, source, level, calls, flags=None):
    d = O.QUAL_DEFAULTS[mode]
    qc = ctx.qual_coder(mode, source, level, d[0], d[1])
    reads = ctx.pack_readset(rs)
    quals = torch.from_numpy(rs.quals).to(ctx.device)
    qoff = torch.from_numpy(rs.offsets).to(ctx.device)
    fl = None if flags is None else torch.from_numpy(flags).to(ctx.device)
    parts = []
    for b in calls:
        out, sizes = qc.encode(reads, quals, qoff, b, fl)
        raw, o = out.cpu().numpy().tobytes(), 0
        for s in sizes:
            parts.append(raw[o:o + s])
            o += s
    qc.free(); reads.free()
    return parts


def oracle_encode(rs, mode, source, level, bounds, flags=None):
    qc = O.QualCoder(True, mode, source, level)
    parts = []
    for pi in range(len(bounds) - 1):
        for i in range(bounds[pi], bounds[pi + 1]):
            f = None if flags is None else flags[rs.offsets[i]:rs.offsets[i + 1]]
            qc.encode(rs.read(i), rs.qual(i), f)
        parts.append(qc.finish_part())
    return parts


@pytest.mark.parametrize("mode", PER_BASE_MODES)
@pytest.mark.parametrize("source,level", [(0, 1), (1, 3)])
def test_short_reads_every_missing_history_slot(ctx, mode, source, level):
    rs = short_and_long_reads(100 + mode, lambda rng, n: np.clip(rng.normal(20, 12, n), 0, 93).astype(np.uint8))
    rng = np.random.default_rng(mode)
    flags = rng.choice(np.frombuffer(b"AM P", np.uint8), len(rs.quals)) if level > 1 else None
    n = rs.n_reads
    bounds = np.array([0, 9, n // 3, n // 3, n - 5, n], dtype=np.int64)
    got = gpu_encode(ctx, rs, mode, source, level, [bounds], flags)
    exp = oracle_encode(rs, mode, source, level, bounds, flags)
    assert [len(p) for p in got] == [len(p) for p in exp]
    assert got == exp


@pytest.mark.parametrize("mode", PER_BASE_MODES)
def test_qualities_over_all_bins(ctx, mode):
    rs = short_and_long_reads(200 + mode, lambda rng, n: rng.integers(0, 94, n).astype(np.uint8))
    n = rs.n_reads
    bounds = np.array([0, n // 2, n], dtype=np.int64)
    assert gpu_encode(ctx, rs, mode, 0, 1, [bounds]) == oracle_encode(rs, mode, 0, 1, bounds)


@pytest.mark.parametrize("mode", [0, 2, 3, 4])
def test_encode_split_over_two_calls(ctx, mode):
    rs = short_and_long_reads(300 + mode, lambda rng, n: np.clip(rng.normal(18, 10, n), 0, 93).astype(np.uint8))
    n = rs.n_reads
    bounds = np.array([0, n // 5, n // 2, n - 7, n], dtype=np.int64)
    one = gpu_encode(ctx, rs, mode, 0, 1, [bounds])
    two = gpu_encode(ctx, rs, mode, 0, 1, [bounds[:3], bounds[2:]])
    assert one == two == oracle_encode(rs, mode, 0, 1, bounds)


@pytest.mark.parametrize("begin,end", [(2, 17), (0, 15), (8, 18), (3, 30), (5, 9), (16, 43)])
def test_sort_ignores_bits_above_end_bit(ctx, begin, end):
    """Keys with non-zero bits everywhere: the result is ordered on bits [begin, end) only, and equal fields keep their input order —
    also where the last digit of the pass plan reaches above `end` (15 bits = 8 + 7, 10 = 8 + 2, 27 = 9 + 9 + 9 ...)."""
    n = 300_007
    gen = torch.Generator().manual_seed(begin * 64 + end)
    keys = torch.randint(0, 1 << 62, (n,), generator=gen, dtype=torch.int64)
    vals = torch.arange(n, dtype=torch.int32)
    field = (keys >> begin) & ((1 << (end - begin)) - 1)
    _, order = torch.sort(field, stable=True)
    dk, dv = keys.to(ctx.device), vals.to(ctx.device)
    ctx.sort_u64(dk, dv, begin, end)
    assert torch.equal(dv.cpu(), vals[order])               # ordered on the field, stable
    assert torch.equal(dk.cpu(), keys[order])               # whole keys travel with it
    dk2 = keys.to(ctx.device)
    ctx.sort_u64(dk2, None, begin, end)
    assert torch.equal(dk2.cpu(), keys[order])
