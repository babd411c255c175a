"""GPU suite of the content report: k_report_bases and k_report_quals of csrc/report.hip — cl_report_bases, cl_report_quals —
against the host forms of the C ABI and tests/report_ref.py (numpy, itself checked in tests/test_report_cpu.py), exactly, on constructed
read sets: every length around an 8-byte group, a 32-base arena word, a 64-lane step and a 512-byte step, one read of 100 000, quality
offsets that are not 8-aligned, N at the edges of the arena words, every quad edge, the grid-stride loop and the flush path at small shapes.
Then the pipeline's hook (cl_ctx_set_report) under the one-call driver and the chunked compressor."""
import ctypes as C
import numpy as np
import pytest
import torch
from colord_amd import _native as N
import digest_ref as R
import report_ref as P
import test_qual_values_cpu as TC
import test_report_cpu as TR

pytestmark = pytest.mark.gpu
LENS = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 100_000]
MODES = TC.ALL_MODES + ["none"]
LEAD = 3


def constructed():
    """(codes, input quality bytes) per read: the edge lengths, then N at positions 0, 31, 32 and last, an all-N read, one read with bytes
    outside Phred+33 0..95, one read with every base in one bin, one of 0 and 95 alternating"""
    rng = np.random.default_rng(17)
    wide = np.array([0, 3, 6, 7, 10, 13, 14, 20, 25, 26, 40, 92, 93, 95], np.uint8)
    quals = [rng.choice(wide, L) if i % 2 else rng.integers(0, 96, L).astype(np.uint8) for i, L in enumerate(LENS)]
    quals += [rng.integers(0, 96, 70).astype(np.uint8), rng.integers(0, 96, 40).astype(np.uint8), np.full(700, 30, np.uint8), np.tile(np.array([0, 95], np.uint8), 300)]
    quals = [(q + 33).astype(np.uint8) for q in quals]
    quals.append(np.array([0, 32, 33, 128, 129, 255, 73, 74, 200], np.uint8))
    codes = [rng.integers(0, 4, len(q)).astype(np.uint8) for q in quals]
    codes[len(LENS)][[0, 31, 32, 69]] = 4
    codes[len(LENS) + 1][:] = 4
    codes[5][31] = 4; codes[6][[31, 32]] = 4; codes[8][[0, 63]] = 4; codes[16][[0, 31, 32, 99_999]] = 4
    return codes, quals


@pytest.fixture(scope="module")
def data():
    return constructed()


_REF = {}


def want(data, mode, T=None, D=None, sel=None):
    """report_ref of the constructed set (a selection of its reads), computed once per case"""
    key = (mode, tuple(T or ()), tuple(D or ()), tuple(sel) if sel is not None else None)
    if key not in _REF:
        codes, quals = data
        if sel is not None:
            codes, quals = [codes[i] for i in sel], [quals[i] for i in sel]
        _REF[key] = P.report(codes, quals, mode, T, D)
    return _REF[key]


def device_input(ctx, codes, quals, lead=LEAD):
    """the arena of the reads; their quality bytes behind `lead` foreign bytes (no read starts 8-aligned by construction) and the offsets"""
    lens = [len(r) for r in codes]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    c = np.concatenate(codes) if codes else np.zeros(0, np.uint8)
    arena = ctx.pack_reads(torch.from_numpy(c), torch.from_numpy(off))
    q = np.concatenate([np.full(lead, 33 + 50, np.uint8)] + list(quals) + [np.full(5, 33 + 60, np.uint8)])
    return arena, torch.from_numpy(q).to(ctx.device), torch.from_numpy(off + lead).to(ctx.device)


def device_report(ctx, codes, quals, mode, T=None, D=None, lead=LEAD, flush_bytes=0, max_blocks=0, acc=None):
    arena, q, qoff = device_input(ctx, codes, quals, lead)
    fwd = R.DEFAULT_T.get(mode, ()) if T is None else T
    rev = R.DEFAULT_D.get(mode, ()) if D is None else D
    try:
        acc = ctx.report_bases(arena, acc)
        return ctx.report_quals(arena, q, qoff, R.QUAL_MODES.index(mode), fwd, rev, flush_bytes, max_blocks, acc)
    finally:
        arena.free()


@pytest.mark.parametrize("mode", MODES)
def test_device_equals_host_equals_reference(ctx, data, mode):
    codes, quals = data
    ref = want(data, mode)
    host = TR.host_report(codes, quals, mode).as_dict()
    assert P.same(host, ref) is None, P.same(host, ref)
    for lead in (LEAD, 0, 5):                                                  # quality offsets 3, 0 and 5 mod 8 at the first read
        got = device_report(ctx, codes, quals, mode, lead=lead).as_dict()
        assert P.same(got, ref) is None, (mode, lead, P.same(got, ref))
    if mode != "none":
        assert ref["q_joint"][0].sum() > 0 and ref["base_count"][4] == 4 + 40 + 1 + 2 + 2 + 4      # the bytes outside 0..95 counted as 0; every N


@pytest.mark.parametrize("mode,T,D", [("4-avg", [5, 5, 30], None), ("5-avg", [3, 9, 9, 96], None), ("2-avg", [96], None), ("2-avg", [0], None), ("4-fix", [5, 5, 30], [40, 41, 42, 43]),
                                      ("5-fix", [3, 9, 9, 96], [0, 95, 7, 9, 11]), ("2-fix", [11], [5, 20])],
                         ids=["4-avg_empty_bin", "5-avg_T96", "2-avg_T96", "2-avg_T0", "4-fix_empty_bin_D", "5-fix_T96_D", "2-fix_D"])
def test_custom_thresholds_and_values(ctx, data, mode, T, D):
    codes, quals = data
    ref = want(data, mode, T, D)
    got = device_report(ctx, codes, quals, mode, T, D).as_dict()
    assert P.same(got, ref) is None, P.same(got, ref)
    assert P.same(TR.host_report(codes, quals, mode, T, D).as_dict(), ref) is None


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("mode", ["4-avg", "5-fix"])
def test_quad_edges(ctx, data, mode, n):
    sel = list(range(9, 9 + n))                                               # lengths 65, 511, 512, 513, 4095, 4096, 4097, 100 000, 70
    codes, quals = [data[0][i] for i in sel], [data[1][i] for i in sel]
    got = device_report(ctx, codes, quals, mode).as_dict()
    ref = want(data, mode, sel=sel)
    assert P.same(got, ref) is None, (mode, n, P.same(got, ref))


@pytest.mark.parametrize("max_blocks", [1, 2, 0])
@pytest.mark.parametrize("flush_bytes", [1, 4096, 0])
@pytest.mark.parametrize("mode", ["4-avg", "org"])
def test_grid_stride_and_flush_paths_give_the_same_matrix(ctx, data, mode, flush_bytes, max_blocks):
    """22 reads are six quads: one and two blocks stride over them; flush_bytes = 1 flushes after every quad, 4096 after most"""
    codes, quals = data
    assert (len(codes) + 3) // 4 > 2
    got = device_report(ctx, codes, quals, mode, flush_bytes=flush_bytes, max_blocks=max_blocks).as_dict()
    assert P.same(got, want(data, mode)) is None, (mode, flush_bytes, max_blocks, P.same(got, want(data, mode)))


@pytest.mark.parametrize("mode", ["org", "4-avg", "2-fix", "avg"])
def test_two_calls_over_halves_add_up(ctx, data, mode):
    codes, quals = data
    ref = want(data, mode)
    cut = 10                                                                   # inside a quad
    acc = device_report(ctx, codes[cut:], quals[cut:], mode, lead=6)
    both = device_report(ctx, codes[:cut], quals[:cut], mode, acc=acc)
    assert P.same(both.as_dict(), ref) is None
    a, b = device_report(ctx, codes[:cut], quals[:cut], mode), device_report(ctx, codes[cut:], quals[cut:], mode, max_blocks=1, flush_bytes=1)
    N.load().cl_report_add(C.byref(a), C.byref(b))
    assert P.same(a.as_dict(), ref) is None
    assert a.len_min == 1 and a.len_max == 100_000


def test_parameters_are_checked_before_any_launch(data):
    from colord_amd.device import Context
    codes, quals = data
    c = Context(0, timing=True)
    try:
        arena, q, qoff = device_input(c, codes[:5], quals[:5])
        acc = c.new_report()
        for mode, fwd, rev in ((6, [7], ()), (6, [7], [1]), (6, [7], [1, 96]), (4, [7, 14, 26, 93], [3, 10, 18, 35, 100]), (2, [7, 14], ())):
            with pytest.raises(N.ColordHipError) as e:
                c.report_quals(arena, q, qoff, mode, fwd, rev, acc=acc)
            assert e.value.status == N.CL_E_INVALID
            assert not [k for k in c.kernel_times() if "k_report" in k]
        assert P.same(acc.as_dict(), P.empty()) is None                        # a refused call adds nothing
        prm = c._qual_params(0, (), ())
        lib = N.load()
        assert lib.cl_report_bases(c.h, None, C.byref(acc)) == N.CL_E_INVALID and lib.cl_report_bases(c.h, arena.h, None) == N.CL_E_INVALID
        assert lib.cl_report_bases(None, arena.h, C.byref(acc)) == N.CL_E_INVALID
        assert lib.cl_report_quals(c.h, None, arena.h, q.data_ptr(), qoff.data_ptr(), 0, 0, C.byref(acc)) == N.CL_E_INVALID
        assert lib.cl_report_quals(c.h, C.byref(prm), None, q.data_ptr(), qoff.data_ptr(), 0, 0, C.byref(acc)) == N.CL_E_INVALID
        assert lib.cl_report_quals(c.h, C.byref(prm), arena.h, None, qoff.data_ptr(), 0, 0, C.byref(acc)) == N.CL_E_INVALID
        assert lib.cl_report_quals(c.h, C.byref(prm), arena.h, q.data_ptr(), None, 0, 0, C.byref(acc)) == N.CL_E_INVALID
        assert lib.cl_report_quals(c.h, C.byref(prm), arena.h, q.data_ptr(), qoff.data_ptr(), 0, 0, None) == N.CL_E_INVALID
        assert P.same(acc.as_dict(), P.empty()) is None
        none = c.report_quals(arena, q, qoff, 8)                               # none: nothing is counted
        assert P.same(none.as_dict(), P.empty()) is None
        arena.free()
    finally:
        c.close()


@pytest.mark.parametrize("name", sorted(TC.CODED))
def test_device_report_of_the_golden_input_is_what_the_reference_archives_decode_to(ctx, name, tmp_path):
    """tests/test_report_cpu.py's pin on the device: the OUT marginal from the first 24 input reads == the histogram of the quality lines
    `colord_hip decompress` (SHA-pinned to the reference's decompressor) returns for the reference-written archive"""
    import hashlib, os, subprocess
    out = str(tmp_path / "o.fastq")
    subprocess.check_call([TC.CLI, "decompress", os.path.join(TC.ARC, name + ".colord"), out], stderr=subprocess.DEVNULL)
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == TC.EXP[name]["decompressed_sha256"]
    recs = R.parse_fastq(out)
    codes, quals = TR.input_records()
    got = device_report(ctx, codes, quals, TC.CODED[name]).as_dict()
    hist = np.bincount(np.concatenate([r[2] for r in recs]).astype(np.int64), minlength=96).astype(np.uint64)
    assert np.array_equal(P.out_marginal(got), hist)
    assert P.same(got, P.report([r[1] for r in recs]), ("reads", "bases", "base_count", "len_min", "len_max", "len_hist", "len_bases")) is None


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------------
def test_drivers_report_their_input_and_only_when_asked():
    """cl_ctx_set_report: the one-call driver and the chunked compressor (two chunkings, one with every chunk announced to the encode lanes) add the
    report of their reads to the context's total and write the parts they write without it; off (the default): the empty report and no k_report_*
    launch."""
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

    def launched():
        return [k for k in set(c.kernel_times()) | set(c.acc) if "k_report" in k]
    try:
        off_one = one_call(c, rs, prm, packs, qual_args)
        assert P.same(c.report().as_dict(), P.empty()) is None and not launched()
        c.set_report(True)
        on_one = one_call(c, rs, prm, packs, qual_args)
        r1 = c.report().as_dict()
        assert launched()
        assert c.digest() == ((0, 0, 0), (0, 0, 0)) and c.digest_values() == (0, 0, 0)      # a flag of its own
        c.set_report(False); c.set_report(True)                               # switched on: cleared
        on_three = chunked(c, rs, prm, packs, even_cuts(len(packs) - 1, 3), qual_args, announce="all")
        r2 = c.report().as_dict()
        on_two = chunked(c, rs, prm, packs, even_cuts(len(packs) - 1, 2), qual_args)
        r3 = c.report().as_dict()                                              # (not cleared in between: twice the input)
        c.set_report(False)
        off_again = one_call(c, rs, prm, packs, qual_args)
        assert P.same(c.report().as_dict(), r3) is None
    finally:
        c.close()
    assert on_one[:4] == off_one[:4] == off_again[:4] and on_three[:4] == off_one[:4] and on_two[:4] == off_one[:4]
    codes = [rs.bases[rs.offsets[i]:rs.offsets[i + 1]] for i in range(rs.n_reads)]
    quals = [rs.quals[rs.offsets[i]:rs.offsets[i + 1]] for i in range(rs.n_reads)]
    ref = P.report(codes, quals, R.QUAL_MODES[qm], list(d[0]) or None, list(d[1]) or None)
    assert P.same(r1, ref) is None and P.same(r2, ref) is None and P.same(r3, P.add(ref, ref)) is None
