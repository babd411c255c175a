"""GPU suite for the model domains of the quality stream: the encoder's reset at a part boundary (cl_qual_coder_set_domain_symbols) is
what a fresh coder does, and the device decoder (cl_qual_decode_domains, one lane per domain) gives byte for byte what the host chain
gives (cl_qual_decode_part with cl_qual_decoder_new_domain at every domain start).  The yardstick is the existing encoder — itself
pinned to the oracle by test_gpu_qual.py — and the existing host decoder."""
import ctypes as C
import numpy as np
import pytest
import torch
from colord_amd import _native as N
from colord_amd.fastq import ReadSet
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

PART_SYMBOLS = 4096
LONG_READ = 9000                       # longer than a part: it is a part of its own
# all nine modes at level 1; org and 4-avg at levels 2 and 3
CASES = [(m, 1) for m in range(9)] + [(0, 2), (2, 2), (0, 3), (2, 3)]
NAVG = {1: 10, 2: 8, 3: 4, 7: 2}


@pytest.fixture(scope="module")
def rs():
    """800 reads of 50 .. 3000 bases, some with N, one of a single base, one longer than a part; qualities over the whole alphabet."""
    rng = np.random.default_rng(77)
    lens = rng.integers(50, 3001, 800)
    lens[rng.integers(0, 800, 500)] //= 8                       # many short reads too
    lens = np.maximum(lens, 50)
    lens[17] = 1
    lens[301] = LONG_READ
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    bases = rng.integers(0, 4, off[-1], dtype=np.uint8)
    for r in rng.integers(0, 800, 60):                          # N in some reads (first and last base included)
        bases[rng.integers(off[r], off[r + 1], 3)] = 4
    bases[off[40]] = 4; bases[off[41 + 1] - 1] = 4
    quals = (33 + np.clip(rng.normal(20, 12, off[-1]), 0, 93).astype(np.uint8)).astype(np.uint8)
    n = len(lens)
    return ReadSet(bases, off, quals, [b"r%d" % i for i in range(n)], [False] * n, True)


@pytest.fixture(scope="module")
def bounds(rs):
    """parts of about 4 Ki bases, cut at read boundaries; the long read is alone in its part"""
    b, acc = [0], 0
    for r in range(rs.n_reads):
        ln = int(rs.offsets[r + 1] - rs.offsets[r])
        if ln == LONG_READ and b[-1] != r:
            b.append(r); acc = 0
        acc += ln
        if acc >= PART_SYMBOLS or ln == LONG_READ:
            b.append(r + 1); acc = 0
    if b[-1] != rs.n_reads:
        b.append(rs.n_reads)
    b = np.array(b, dtype=np.int64)
    assert any(b[i + 1] - b[i] == 1 and rs.offsets[b[i + 1]] - rs.offsets[b[i]] == LONG_READ for i in range(len(b) - 1))
    return b


@pytest.fixture(scope="module")
def flags(rs):
    return np.random.default_rng(3).choice(np.frombuffer(b"AM P", np.uint8), len(rs.quals))


def part_symbols(rs, bounds, mode):
    """coded symbols of every part: one per base (not avg, none) and the average bytes of every read"""
    o = rs.offsets
    per_base = 0 if mode in (7, 8) else 1
    return [int(per_base * (o[bounds[p + 1]] - o[bounds[p]]) + NAVG.get(mode, 0) * (bounds[p + 1] - bounds[p])) for p in range(len(bounds) - 1)]


def expected_starts(syms, n):
    """a part opens a domain when the open one holds n symbols or more"""
    out, since = [0], 0
    for p, s in enumerate(syms):
        if n and since >= n:
            out.append(p); since = 0
        since += s
    return out


def subset(rs, r0, r1):
    o = rs.offsets
    return ReadSet(rs.bases[o[r0]:o[r1]], (o[r0:r1 + 1] - o[r0]).astype(np.int64), rs.quals[o[r0]:o[r1]], rs.headers[r0:r1], [False] * (r1 - r0), True)


def encode(ctx, rs, mode, level, bounds, flags=None, dom_n=None, split=None):
    """-> (parts, domain starts) of one coder over the reads; dom_n None: the setting is never touched; split: two calls"""
    d = O.QUAL_DEFAULTS[mode]
    qc = ctx.qual_coder(mode, 0, level, d[0], d[1])
    if dom_n is not None:
        qc.set_domain_symbols(dom_n)
    reads = ctx.pack_readset(rs)
    quals = torch.from_numpy(rs.quals).to(ctx.device)
    qoff = torch.from_numpy(rs.offsets).to(ctx.device)
    fl = None if flags is None or level <= 1 else torch.from_numpy(np.ascontiguousarray(flags)).to(ctx.device)
    parts = []
    for b in ([bounds] if split is None else [bounds[:split + 1], bounds[split:]]):
        out, sizes = qc.encode(reads, quals, qoff, b, fl)
        raw, o = out.cpu().numpy().tobytes(), 0
        for s in sizes:
            parts.append(raw[o:o + s]); o += s
    doms = qc.domains()
    qc.free(); reads.free()
    return parts, doms


_CODED = {}


def coded(ctx, rs, bounds, flags, mode, level):
    """the parts of (mode, level) with domains of about a fifth of the stream, made once for the tests that need them"""
    key = (mode, level)
    if key not in _CODED:
        syms = part_symbols(rs, bounds, mode)
        n = max(1, sum(syms) // 5)
        parts, doms = encode(ctx, rs, mode, level, bounds, flags, n)
        _CODED[key] = (n, parts, doms)
    return _CODED[key]


def host_chain(rs, parts, bounds, starts, mode, level, flags=None, digest=False):
    """cl_qual_decode_part over the parts with cl_qual_decoder_new_domain at every domain start -> (qualities, digest triple)"""
    lib = N.load()
    d = O.QUAL_DEFAULTS[mode]
    prm = N.QualParams(mode=mode, source=0, level=level, n_fwd=len(d[0]), n_rev=len(d[1]))
    for i, v in enumerate(d[0]):
        prm.fwd[i] = v
    for i, v in enumerate(d[1]):
        prm.rev[i] = v
    q = N._P()
    assert lib.cl_qual_decoder_create(C.byref(prm), C.byref(q)) == 0
    if digest:
        assert lib.cl_qual_decoder_set_digest(q, 1, 0) == 0
    bases = rs.bases.copy()
    if level > 1:                                                   # the class flags as cl_dna_decode_part hands them on
        bases[flags == ord("A")] |= 0x80
        bases[flags == ord("M")] |= 0x40
    o = rs.offsets
    out = np.zeros(len(bases), np.uint8)
    for p, payload in enumerate(parts):
        if p and p in starts:
            assert lib.cl_qual_decoder_new_domain(q) == 0
        r0, r1 = int(bounds[p]), int(bounds[p + 1])
        b = np.ascontiguousarray(bases[o[r0]:o[r1]]); off = (o[r0:r1 + 1] - o[r0]).astype(np.uint64)
        res = np.zeros(max(len(b), 1), np.uint8); buf = np.frombuffer(payload, np.uint8)
        assert lib.cl_qual_decode_part(q, buf.ctypes.data, len(buf), b.ctypes.data, off.ctypes.data, r1 - r0, res.ctypes.data) == 0
        out[o[r0]:o[r1]] = res[:len(b)]
    dg = N.Digest()
    assert lib.cl_qual_decoder_digest(q, C.byref(dg)) == 0
    lib.cl_qual_decoder_free(q)
    return out, dg.triple()


def device_decode(ctx, rs, parts, bounds, starts, mode, level, flags=None, max_domains=0, want_symbols=False):
    d = O.QUAL_DEFAULTS[mode]
    reads = ctx.pack_readset(rs)
    payload = torch.from_numpy(np.frombuffer(b"".join(parts), np.uint8).copy()).to(ctx.device)
    qoff = torch.from_numpy(rs.offsets).to(ctx.device)
    fl = None if level <= 1 else torch.from_numpy(np.ascontiguousarray(flags)).to(ctx.device)
    try:
        return ctx.qual_decode_domains(mode, 0, level, d[0], d[1], reads, payload, bounds, [len(p) for p in parts], starts, qoff, fl, max_domains, want_symbols)
    finally:
        reads.free()


# ---- 1. the reset is what a fresh coder does ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,level", CASES)
def test_a_domain_is_coded_as_by_a_fresh_coder(ctx, rs, bounds, flags, mode, level):
    syms = part_symbols(rs, bounds, mode)
    n, parts, doms = coded(ctx, rs, bounds, flags, mode, level)
    assert doms == expected_starts(syms, n)
    if mode == 8:
        assert doms == [0]                                           # nothing is coded: a domain never fills
    else:
        assert len(doms) >= 3 and all(b - a >= 2 for a, b in zip(doms, doms[1:]))
    plain, plain_doms = encode(ctx, rs, mode, level, bounds, flags)  # a coder whose setting is never touched: the bytes as they always were
    assert plain_doms == [0]
    zero, zero_doms = encode(ctx, rs, mode, level, bounds, flags, 0)
    assert zero == plain and zero_doms == [0]
    ends = doms[1:] + [len(parts)]
    assert parts[:ends[0]] == plain[:ends[0]]
    for a, b in zip(doms[1:], ends[1:]):
        r0, r1 = int(bounds[a]), int(bounds[b])
        sub = subset(rs, r0, r1)
        fresh, _ = encode(ctx, sub, mode, level, bounds[a:b + 1] - r0, flags[rs.offsets[r0]:rs.offsets[r1]])
        assert parts[a:b] == fresh, (a, b)


def test_domains_count_parts_over_the_coders_lifetime(ctx, rs, bounds, flags):
    """two calls: the same bytes and the same starts as one (a domain may begin with a call, or span two)"""
    n, parts, doms = coded(ctx, rs, bounds, flags, 2, 1)
    for split in (doms[1], doms[2] + 1):
        assert encode(ctx, rs, 2, 1, bounds, None, n, split=split) == (parts, doms)


# ---- 2. device decode equals host decode -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,level", CASES)
def test_device_decode_equals_host_chain(ctx, rs, bounds, flags, mode, level):
    n, parts, doms = coded(ctx, rs, bounds, flags, mode, level)
    exp, exp_digest = host_chain(rs, parts, bounds, doms, mode, level, flags, digest=True)
    got, (syms, sym_off) = device_decode(ctx, rs, parts, bounds, doms, mode, level, flags, want_symbols=True)
    got = got.cpu().numpy()
    assert np.array_equal(got, exp)
    if mode == 0:
        assert np.array_equal(got, rs.quals)
    if mode != 8:                                                   # (none: nothing is coded, nothing digested)
        lib = N.load()
        h = np.ascontiguousarray(syms.cpu().numpy()); acc = N.Digest()
        assert lib.cl_digest_bytes_host(2, h.ctypes.data, sym_off.ctypes.data, rs.n_reads, 0, C.byref(acc)) == 0
        reads = ctx.pack_readset(rs)
        d = O.QUAL_DEFAULTS[mode]
        want = ctx.digest_quals(reads, torch.from_numpy(rs.quals).to(ctx.device), torch.from_numpy(rs.offsets).to(ctx.device), mode, d[0], 0)
        reads.free()
        assert acc.triple() == tuple(want) == exp_digest


# ---- 3. shapes ---------------------------------------------------------------------------------------------------------------------------
def test_one_domain(ctx, rs, bounds):
    parts, doms = encode(ctx, rs, 2, 1, bounds)
    assert doms == [0]
    exp, _ = host_chain(rs, parts, bounds, doms, 2, 1)
    assert np.array_equal(device_decode(ctx, rs, parts, bounds, doms, 2, 1).cpu().numpy(), exp)


@pytest.mark.parametrize("mode", [0, 2])
def test_seventy_domains_of_one_part(ctx, rs, bounds, mode):
    """more than a wave and a partial one; every domain a single part (the single-read part and the read of one base among them)"""
    b = bounds[:71]
    sub = subset(rs, 0, int(b[-1]))
    parts, doms = encode(ctx, sub, mode, 1, b, None, 1)
    assert doms == list(range(70))
    assert any(b[i] <= 17 < b[i + 1] for i in range(70))            # the read of length 1
    exp, _ = host_chain(sub, parts, b, doms, mode, 1)
    assert np.array_equal(device_decode(ctx, sub, parts, b, doms, mode, 1).cpu().numpy(), exp)


def test_batch_limit_takes_several_launches(ctx, rs, bounds, flags):
    """8 domains, at most 3 a launch: three launches, the last one short"""
    syms = part_symbols(rs, bounds, 2)
    n = 10_000
    starts = expected_starts(syms, n)
    assert len(starts) > 8
    b = bounds[:starts[8] + 1]
    sub = subset(rs, 0, int(b[-1]))
    parts, doms = encode(ctx, sub, 2, 1, b, None, n)
    assert doms == starts[:8]
    exp, _ = host_chain(sub, parts, b, doms, 2, 1)
    assert np.array_equal(device_decode(ctx, sub, parts, b, doms, 2, 1, max_domains=3).cpu().numpy(), exp)


# ---- 4. bad input is refused and never wandered through ----------------------------------------------------------------------------------
def test_a_shortened_part_is_refused_by_name(ctx, rs, bounds, flags):
    """One part loses its last 3 bytes (in the size table and in the payload): the decoder reads zeros past the part's size — never the
    next part's bytes — and the part then does not end at its size.  The other domains are decoded completely."""
    n, parts, doms = coded(ctx, rs, bounds, flags, 2, 1)
    exp, _ = host_chain(rs, parts, bounds, doms, 2, 1)
    k = doms[1] + 1                                                 # the second part of domain 1
    assert k < doms[2] - 0
    cut = list(parts); cut[k] = cut[k][:-3]
    with pytest.raises(N.ColordHipError) as ei:
        device_decode(ctx, rs, cut, bounds, doms, 2, 1)
    assert ei.value.status == N.CL_E_MISMATCH
    assert "domain 1," in str(ei.value) and f"part {k} " in str(ei.value)
    got = ei.value.quals.cpu().numpy()
    o = rs.offsets
    lo, hi = int(o[bounds[doms[1]]]), int(o[bounds[doms[2]]])
    assert np.array_equal(got[:lo], exp[:lo]) and np.array_equal(got[hi:], exp[hi:])
    assert np.array_equal(got[lo:int(o[bounds[k]])], exp[lo:int(o[bounds[k]])])      # the part before it in the same domain


# ---- 5. domains long enough for the models to rescale ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2, 6])
def test_hot_contexts_rescale_inside_a_domain(ctx, mode):
    """Long reads of one base and one quality value: nearly every symbol of a domain falls into ONE context, far more often than the 32 768
    updates after which a model halves its counts (adder 8 at a total of 2^18; org: 32 at 2^20; rc.h:233-244) — the decoder's rescale
    runs many times per domain, in the per-base family and (4-avg) with the same averages read after read.  Three domains of two parts."""
    rng = np.random.default_rng(5)
    lens = [120_000] * 6 + [1, 64, 65]
    bases = np.concatenate([np.full(l, i % 4, np.uint8) for i, l in enumerate(lens)])
    quals = np.concatenate([np.full(l, 33 + (5, 20, 30, 10)[i % 4], np.uint8) for i, l in enumerate(lens)])
    spots = rng.integers(0, len(quals), 2000)
    quals[spots] = 33 + 40
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    hot = ReadSet(bases, off, quals, [b"r%d" % i for i in range(len(lens))], [False] * len(lens), True)
    b = np.array([0, 1, 2, 3, 4, 5, len(lens)], dtype=np.int64)
    assert (120_000 - 6 * 2000) * 2 > 4 * 32_768                      # the hot context of a domain, whatever the spots do to its neighbours
    parts, doms = encode(ctx, hot, mode, 1, b, None, 200_000)
    assert doms == [0, 2, 4]
    exp, _ = host_chain(hot, parts, b, doms, mode, 1)
    got = device_decode(ctx, hot, parts, b, doms, mode, 1).cpu().numpy()
    assert np.array_equal(got, exp)
    if mode == 0:
        assert np.array_equal(got, hot.quals)
