"""GPU suite of the qual-values digest (kind 4): k_qual_values of csrc/digest.hip — cl_qual_values (the bytes) and
cl_digest_qual_values (the triple) — against tests/qual_values_ref.py (numpy, from the definition, itself checked in
tests/test_qual_values_cpu.py), on hand-made inputs chosen where the kernel can go wrong: every length around an 8-byte group and a
512-byte step, quality offsets that are not 8-aligned, partial blocks, empty bins, one read that carries its counters through
hundreds of steps with k A beyond 2^32.  Then the reference-written archives' decoded lines from their input reads on the device, and
the pipeline's hook (cl_ctx_set_digest_values)."""
import numpy as np
import pytest
import torch
from colord_amd import _native as N
import digest_ref as R
import qual_values_ref as V
import test_qual_values_cpu as TC

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
LENS = [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1025]
MODES = TC.ALL_MODES
GUARD, LEAD = 0xEE, 3


def hand_made():
    """input quality reads (ASCII): the edge lengths back to back, every base in one bin, bins alternating every base, 0 and 95"""
    rng = np.random.default_rng(31)
    wide = np.array([0, 3, 6, 7, 10, 13, 14, 20, 25, 26, 40, 92, 93, 95], np.uint8)
    reads = [rng.choice(wide, L) for L in LENS]
    reads.append(np.full(700, 30, np.uint8))
    reads.append(np.tile(np.array([2, 40], np.uint8), 300))
    reads.append(np.array([0, 95, 0, 95, 95, 0, 0, 95, 95], np.uint8))
    reads += [rng.integers(0, 96, int(L)).astype(np.uint8) for L in rng.integers(1, 900, 6)]
    return [(r + 33).astype(np.uint8) for r in reads]


@pytest.fixture(scope="module")
def reads():
    return hand_made()


def device_input(ctx, reads_ascii, lead=LEAD):
    """the reads' quality bytes behind `lead` foreign bytes (so that no read starts 8-aligned by construction), their offsets, an arena of as many reads"""
    lens = [len(r) for r in reads_ascii]
    q = np.concatenate([np.full(lead, 33 + 50, np.uint8)] + list(reads_ascii)) if reads_ascii else np.full(lead, 33 + 50, np.uint8)
    off = (lead + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)
    codes = np.zeros(int(sum(lens)), np.uint8)
    arena = ctx.pack_reads(torch.from_numpy(codes), torch.from_numpy((off - lead).astype(np.int64)))
    return arena, torch.from_numpy(q).to(ctx.device), torch.from_numpy(off).to(ctx.device), off


def run(ctx, reads_ascii, mode, T=None, D=None, first=0, lead=LEAD):
    """-> (per read the bytes cl_qual_values stored, the triple of cl_digest_qual_values); the bytes around the values must be untouched"""
    arena, quals, qoff, off = device_input(ctx, reads_ascii, lead)
    fwd = R.DEFAULT_T.get(mode, ()) if T is None else T
    rev = R.DEFAULT_D.get(mode, ()) if D is None else D
    m = R.QUAL_MODES.index(mode)
    buf = torch.full((int(off[-1]) + 64,), GUARD, dtype=torch.uint8, device=ctx.device)
    ctx.qual_values(arena, quals, qoff, m, fwd, rev, out=buf[:int(off[-1])])
    triple = ctx.digest_qual_values(arena, quals, qoff, m, fwd, rev, first)
    arena.free()
    h = buf.cpu().numpy()
    assert (h[:lead] == GUARD).all() and (h[int(off[-1]):] == GUARD).all(), "bytes outside the reads were written"
    return [h[off[i]:off[i + 1]] for i in range(len(reads_ascii))], triple


def want(reads_ascii, mode, T=None, D=None):
    return [V.values_int(mode, r.astype(np.int64) - 33, T, D) for r in reads_ascii]


def same_bytes(got, exp, what):
    for i, (g, w) in enumerate(zip(got, exp)):
        assert np.array_equal(g, (w.astype(np.int64) + 33).astype(np.uint8)), (what, i, len(w))


@pytest.mark.parametrize("mode", MODES)
def test_values_and_digest_equal_the_reference(ctx, reads, mode):
    exp = want(reads, mode)
    got, triple = run(ctx, reads, mode, first=5)
    same_bytes(got, exp, mode)
    assert triple == V.digest_values(exp, 5)
    _, t0 = run(ctx, reads, mode, first=0, lead=0)                            # (and 8-aligned at the first read)
    assert t0 == V.digest_values(exp, 0)
    _, t40 = run(ctx, reads, mode, first=1 << 40, lead=5)
    assert t40 == V.digest_values(exp, 1 << 40)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5])
@pytest.mark.parametrize("mode", ["4-avg", "5-fix"])
def test_partial_blocks(ctx, reads, mode, n):
    sel = reads[8:8 + n]                                                      # lengths 511, 512, 513, 1025, 700
    exp = want(sel, mode)
    got, triple = run(ctx, sel, mode, first=9)
    same_bytes(got, exp, (mode, n))
    assert triple == V.digest_values(exp, 9)
    if n == 0:
        assert triple == (0, 0, 0)


@pytest.mark.parametrize("mode,T,D", [("4-avg", [5, 5, 30], None), ("5-avg", [3, 9, 9, 96], None), ("2-avg", [96], None), ("2-avg", [0], None), ("4-fix", [5, 5, 30], [40, 41, 42, 43]),
                                      ("5-fix", [3, 9, 9, 96], [0, 222, 7, 9, 11]), ("2-fix", [11], [5, 20])],
                         ids=["4-avg_empty_bin", "5-avg_T96", "2-avg_T96", "2-avg_T0", "4-fix_empty_bin_D", "5-fix_T96_D", "2-fix_D"])
def test_custom_thresholds_and_values(ctx, reads, mode, T, D):
    exp = want(reads, mode, T, D)
    got, triple = run(ctx, reads, mode, T, D, first=2)
    same_bytes(got, exp, (mode, T, D))
    assert triple == V.digest_values(exp, 2)


@pytest.mark.parametrize("mode", ["avg", "2-avg"])
def test_a_long_read_of_high_qualities(ctx, mode):
    """200 000 bases of quality >= 90: k A passes 2^32 (from k = 176 603 at A = 24 320) and the carried counters leave the packed word's ten
    bits behind hundreds of times; two short reads share the launch."""
    rng = np.random.default_rng(5)
    big = (rng.integers(90, 96, 200_000) + 33).astype(np.uint8)
    sel = [hand_made()[4], big, hand_made()[7]]
    exp = want(sel, mode)
    assert 200_000 * V.average_A(big.astype(np.int64) - 33, np.zeros(len(big), np.int64), 1)[0] > 1 << 32
    got, triple = run(ctx, sel, mode, first=1 << 40)
    same_bytes(got, exp, mode)
    assert triple == V.digest_values(exp, 1 << 40)


@pytest.mark.parametrize("mode", ["org", "4-avg", "2-fix", "avg"])
def test_two_calls_over_halves_add_up(ctx, reads, mode):
    exp = want(reads, mode)
    m, fwd, rev = R.QUAL_MODES.index(mode), R.DEFAULT_T.get(mode, ()), R.DEFAULT_D.get(mode, ())
    cut = 10                                                                   # inside a block of four reads
    _, whole = run(ctx, reads, mode, first=7)
    arena_a, qa, oa, _ = device_input(ctx, reads[:cut])
    arena_b, qb, ob, _ = device_input(ctx, reads[cut:], lead=6)
    acc = N.Digest()
    ctx.digest_qual_values(arena_b, qb, ob, m, fwd, rev, 7 + cut, acc)
    two = ctx.digest_qual_values(arena_a, qa, oa, m, fwd, rev, 7, acc)
    arena_a.free(); arena_b.free()
    assert two == whole == V.digest_values(exp, 7)


def test_capacity_and_parameters_are_checked_before_any_launch(ctx, reads):
    arena, quals, qoff, off = device_input(ctx, reads)
    buf = torch.full((int(off[-1]),), GUARD, dtype=torch.uint8, device=ctx.device)
    with pytest.raises(N.ColordHipError) as e:
        ctx.qual_values(arena, quals, qoff, 2, R.DEFAULT_T["4-avg"], (), out=buf[:int(off[-1]) - 1])      # one byte short
    assert e.value.status == N.CL_E_CAPACITY
    assert (buf.cpu().numpy() == GUARD).all()
    with pytest.raises(N.ColordHipError) as e:                                # *-fix without its -D values
        ctx.digest_qual_values(arena, quals, qoff, 6, [7], ())
    assert e.value.status == N.CL_E_INVALID
    with pytest.raises(N.ColordHipError, match="2\\^63"):
        ctx.digest_qual_values(arena, quals, qoff, 0, (), (), (1 << 63) - 1)
    assert ctx.digest_qual_values(arena, quals, qoff, 8) == (0, 0, 0)          # none: nothing is digested
    arena.free()


@pytest.mark.parametrize("name", sorted(TC.CODED))
def test_device_values_of_the_golden_input_are_what_the_reference_archives_decode_to(ctx, name, tmp_path):
    """tests/test_qual_values_cpu.py's check on the device: the first 24 input reads through k_qual_values == the quality lines that
    `colord_hip decompress` (SHA-pinned to the reference's decompressor) returns for the reference-written archive"""
    import hashlib, os, subprocess
    out = str(tmp_path / "o.fastq")
    subprocess.check_call([TC.CLI, "decompress", os.path.join(TC.ARC, name + ".colord"), out], stderr=subprocess.DEVNULL)
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == TC.EXP[name]["decompressed_sha256"]
    lines = [(r[2] + 33).astype(np.uint8) for r in R.parse_fastq(out)]
    got, triple = run(ctx, TC.input_reads(), TC.CODED[name])
    for i in range(24):
        assert np.array_equal(got[i], lines[i]), (name, i)
    assert triple == V.digest_values([(x.astype(np.int64) - 33).astype(np.uint8) for x in lines])


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------------
def sub(a, b):
    return tuple((x - y) & M64 for x, y in zip(a, b))


def test_drivers_digest_the_values_of_their_input_and_only_when_asked():
    """cl_ctx_set_digest_values: the one-call driver and the chunked compressor (two chunkings) add the qual-values digest of their reads, at global
    indices, to the context's total and write the parts they write without it; off (the default): zeroes and no k_qual_values launch."""
    from util import golden
    from bench import reference_part_bounds
    from oracle import pyoracle as O
    from colord_amd.device import Context
    from test_gpu_stream import params_of, one_call, chunked, even_cuts
    g = golden("s6m_ont")
    rs, prm = g.reads, params_of(g)
    packs = reference_part_bounds(np.diff(rs.offsets).astype(np.uint32), 1 << 19)
    qm = g.p("qual_mode"); d = O.QUAL_DEFAULTS[qm]
    qual_args = (qm, g.p("source"), g.p("level"), tuple(d[0]), tuple(d[1]))
    c = Context(0, timing=True)
    try:
        off_one = one_call(c, rs, prm, packs, qual_args)
        assert c.digest_values() == (0, 0, 0)
        assert not [k for k in c.kernel_times() if "k_qual_values" in k] and not [k for k in c.acc if "k_qual_values" in k]
        c.set_digest_values(True)
        on_one = one_call(c, rs, prm, packs, qual_args)
        d1 = c.digest_values()
        assert [k for k in set(c.kernel_times()) | set(c.acc) if "k_qual_values" in k]
        assert c.digest() == ((0, 0, 0), (0, 0, 0))                            # a flag of its own: the other digests stay off
        on_three = chunked(c, rs, prm, packs, even_cuts(len(packs) - 1, 3), qual_args, announce="all")
        d2 = c.digest_values()
        on_two = chunked(c, rs, prm, packs, even_cuts(len(packs) - 1, 2), qual_args)
        d3 = c.digest_values()
        c.set_digest_values(False)
        off_again = one_call(c, rs, prm, packs, qual_args)
        assert c.digest_values() == d3
    finally:
        c.close()
    assert on_one[:4] == off_one[:4] == off_again[:4] and on_three[:4] == off_one[:4] and on_two[:4] == off_one[:4]
    phred = [rs.quals[rs.offsets[i]:rs.offsets[i + 1]].astype(np.int64) - 33 for i in range(rs.n_reads)]
    ref = V.digest_input(R.QUAL_MODES[qm], phred, 0, list(d[0]) or None, list(d[1]) or None)
    assert d1 == ref and sub(d2, d1) == ref and sub(d3, d2) == ref
