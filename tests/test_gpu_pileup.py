"""GPU suite of the pileup (csrc/pileup.hip): k_pileup_walk, k_pileup_fold and k_pileup_sites against their host twin (cl_pileup_host)
and against tests/pileup_ref.py — column for column, site for site, total for total — on the constructed cases of tests/pileupcases.py: the
hand-made streams of tests/editstreams.py over 69 one-piece sequences, and the groups over the nine sequences; read counts 0, 1, 4, 5 and 1025 on one
block; two adds against one; the refusals after finish; the capacity protocol of the sites; malformed streams that stay inside every buffer and spoil
the table; a geometry that does not fit the arena; and the refusals of cl_ctx_set_pileup."""
import ctypes as C
import numpy as np
import pytest
from util import golden
from colord_amd import _native as N
import editstreams as ES
import pileup_ref as PR
import pileupcases as PC
from test_pileup_cpu import host_pileup
from test_gpu_edits import readset_of, to_device
from test_gpu_stream import params_of
from test_gpu_mappings import compressor_with_pseudo_reads, SEQ_LEN, READ_LEN, OVERLAP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hand(ctx):
    case, names = PC.hand()
    refs = ctx.pack_readset(readset_of(case.refs))
    yield case, refs
    refs.free()


@pytest.fixture(scope="module")
def nine(ctx):
    refs = ctx.pack_readset(readset_of(PC.nine([]).refs))
    yield refs
    refs.free()


def device_pileup(ctx, case, refs, batches, max_blocks=0):
    """the table of `batches` of streams, finished"""
    p = ctx.pileup(refs, case.seq_len, case.read_len, case.overlap)
    try:
        for b in batches:
            es, off = to_device(list(b), ctx.device)
            p.add(refs, es, off, max_blocks)
        p.finish()
    except Exception:
        p.free()
        raise
    return p


def same_as_the_judge(p, case, streams, thresholds, who):
    J = case.judged(streams)
    assert p.n_pos == J.n_pos
    cols = p.columns()
    bad = np.nonzero((cols != J.columns()).any(1))[0]
    assert len(bad) == 0, (who, bad[:5].tolist(), cols[bad[:5]].tolist(), J.columns()[bad[:5]].tolist())
    assert p.totals() == J.totals(), who
    for thr in thresholds:
        st, h_cols, h_sites, h_sums, _, _ = host_pileup(case, streams, thr)
        assert st == N.CL_OK and np.array_equal(h_cols, cols) and h_sums == J.totals(), (who, thr)
        got, want = p.sites(*thr), J.sites(*thr)
        assert got.shape == want.shape and np.array_equal(got, want) and np.array_equal(h_sites, want), (who, thr)


def test_hand_made_streams(ctx, hand):
    """every stream of tests/editstreams.py in one batch: 72 898 positions, more than one tile per wave of the fold, and the sites' places from the scan"""
    case, refs = hand
    p = device_pileup(ctx, case, refs, [case.streams])
    try:
        same_as_the_judge(p, case, case.streams, [PR.DEFAULTS, (1, 1, 0), (2, 1, 500)], "hand")
        assert len(p.sites(1, 1, 0)) > 600                                              # (more sites than a tile holds positions)
    finally:
        p.free()


@pytest.mark.parametrize("name", sorted(PC.groups()) + ["everything"])
def test_constructed_groups(ctx, nine, name):
    streams = PC.everything() if name == "everything" else PC.groups()[name]
    case = PC.nine(streams)
    p = device_pileup(ctx, case, nine, [streams])
    try:
        same_as_the_judge(p, case, streams, PC.THRESHOLDS, name)
    finally:
        p.free()


@pytest.mark.parametrize("n", PC.READ_COUNTS)
def test_read_counts_on_one_block(ctx, nine, n):
    """0, 1, 4, 5 and 1025 reads with max_blocks = 1: a block of four waves strides over all of them"""
    pool = PC.everything()
    streams = (pool * (n // len(pool) + 1))[:n]
    case = PC.nine(streams)
    p = device_pileup(ctx, case, nine, [streams], max_blocks=1)
    try:
        same_as_the_judge(p, case, streams, [PR.DEFAULTS, (1, 1, 0)], n)
    finally:
        p.free()


def test_two_adds_equal_one(ctx, nine):
    streams = PC.everything()
    case = PC.nine(streams)
    one, two = device_pileup(ctx, case, nine, [streams]), device_pileup(ctx, case, nine, [streams[:37], [], streams[37:]])
    try:
        assert np.array_equal(one.columns(), two.columns()) and one.totals() == two.totals() and np.array_equal(one.sites(1, 1, 0), two.sites(1, 1, 0))
        same_as_the_judge(two, case, streams, [PR.DEFAULTS], "two adds")
    finally:
        one.free(); two.free()


def test_the_order_of_the_calls_is_kept(ctx, nine):
    streams = PC.groups()["thresholds"]
    case = PC.nine(streams)
    p = ctx.pileup(nine, case.seq_len, case.read_len, case.overlap)
    try:
        es, off = to_device(streams, ctx.device)
        p.add(nine, es, off)
        for call in (p.columns, p.sites, p.totals):                                      # nothing is handed out before finish
            with pytest.raises(N.ColordHipError) as x:
                call()
            assert x.value.status == N.CL_E_INVALID and "after cl_pileup_finish" in str(x.value)
        p.finish()
        with pytest.raises(N.ColordHipError) as x:
            p.add(nine, es, off)
        assert x.value.status == N.CL_E_INVALID and "after cl_pileup_finish" in str(x.value)
        with pytest.raises(N.ColordHipError) as x:
            p.finish()
        assert x.value.status == N.CL_E_INVALID and "twice" in str(x.value)
        same_as_the_judge(p, case, streams, [PR.DEFAULTS], "after the refusals")        # the refused calls changed nothing
        with pytest.raises(N.ColordHipError) as x:
            p.columns(PC.N_POS - 1, 2)
        assert x.value.status == N.CL_E_INVALID
        assert p.columns(PC.N_POS, 0).shape == (0, 8) and p.columns(PC.N_POS - 1, 1).shape == (1, 8)
    finally:
        p.free()


def test_capacity_protocol(ctx, nine):
    """too little room: the need is reported and nothing is written; exactly enough: the sites, and the record behind them stays"""
    streams = PC.everything()
    case = PC.nine(streams)
    want = case.judged().sites(1, 1, 0)
    assert len(want) > 64
    p = device_pileup(ctx, case, nine, [streams])
    try:
        need = C.c_uint64(0)
        out = np.full((len(want) + 1, 12), 0x5a5a5a5a, np.uint32)
        for cap in (0, 1, len(want) - 1):
            st = ctx.lib.cl_pileup_sites(p.h, 1, 1, 0, out.ctypes.data, cap, C.byref(need))
            assert st == N.CL_E_CAPACITY and need.value == len(want) and (out == 0x5a5a5a5a).all()
        with pytest.raises(N.ColordHipError) as x:
            p.sites(1, 1, 0, cap=len(want) - 1)
        assert x.value.status == N.CL_E_CAPACITY and "need %d records" % len(want) in str(x.value)
        st = ctx.lib.cl_pileup_sites(p.h, 1, 1, 0, out.ctypes.data, len(want), C.byref(need))
        assert st == N.CL_OK and need.value == len(want) and np.array_equal(out[:len(want)], want) and (out[len(want)] == 0x5a5a5a5a).all()
        st = ctx.lib.cl_pileup_sites(p.h, 1 << 31, 0, 0, None, 0, C.byref(need))           # no site: nothing is needed
        assert st == N.CL_OK and need.value == 0
    finally:
        p.free()


@pytest.mark.parametrize("name", sorted(ES.malformed_device()))
def test_malformed_stream_is_refused_and_spoils_the_table(ctx, hand, name):
    case, refs = hand
    bad, why = ES.malformed_device()[name]
    good = [case.streams[3], case.streams[40], case.streams[41], case.streams[-2], case.streams[-1]]
    p = ctx.pileup(refs, case.seq_len, case.read_len, case.overlap)
    try:
        es, off = to_device(good[:4] + [bad] + good[4:], ctx.device)
        with pytest.raises(N.ColordHipError) as x:
            p.add(refs, es, off)
        assert x.value.status == N.CL_E_INVALID and "read 4: " + why in str(x.value) and "spoiled" in str(x.value), str(x.value)
        st, _, _, _, bad_read, code = host_pileup(case, good[:4] + [bad] + good[4:])
        assert st == N.CL_E_INVALID and bad_read == 4 and ctx.lib.cl_edit_profile_error(code).decode() == why
        es, off = to_device(good, ctx.device)
        for call in (lambda: p.add(refs, es, off), p.finish, p.columns, p.sites, p.totals):
            with pytest.raises(N.ColordHipError) as x:
                call()
            assert x.value.status == N.CL_E_INVALID and "spoiled" in str(x.value), str(x.value)
    finally:
        p.free()


def test_a_geometry_that_does_not_fit_the_arena_is_refused(ctx, nine):
    G = PC.nine([])
    for seq_len, read_len, overlap, status, text in (
            (G.seq_len, 110, 30, N.CL_E_INVALID, "pseudo read 0 has 100 bases, the geometry gives 110"),      # pieces the arena has reads for, of other lengths
            (G.seq_len[:-1] + [70], 100, 30, N.CL_E_INVALID, "pseudo read 19 has 69 bases, the geometry gives 70"),
            (G.seq_len + [500] * 3, 100, 30, N.CL_E_INVALID, "pieces, the arena has 23 reads"),              # more pieces than the arena has reads
            (G.seq_len, 30, 30, N.CL_E_INVALID, "exceed the overlap"),
            ([1 << 32], 100, 30, N.CL_E_UNSUPPORTED, "2^32"),
            ([(1 << 32) - 1, 1], 1 << 31, 30, N.CL_E_UNSUPPORTED, "2^32")):                                    # sequences that fit, a table that does not
        with pytest.raises(N.ColordHipError) as x:
            ctx.pileup(nine, seq_len, read_len, overlap)
        assert x.value.status == status and text in str(x.value), str(x.value)
    other =ctx.pack_readset(readset_of(G.refs))
    p = ctx.pileup(nine, G.seq_len, G.read_len, G.overlap)
    try:
        es, off = to_device(PC.groups()["thresholds"], ctx.device)
        with pytest.raises(N.ColordHipError) as x:                                      # an arena the lengths were not checked against
            p.add(other, es, off)
        assert x.value.status == N.CL_E_INVALID and "not the arena" in str(x.value)
        p.finish()
        assert p.totals() == dict.fromkeys(PR.TOTALS, 0) and not p.columns()[:, :7].any()
        assert np.array_equal(p.columns()[:, 7], np.concatenate(G.seqs))               # `ref` is filled with no read at all
        empty = ctx.pileup(nine, [], 100, 30)                                           # no sequence: a table of no position
        empty.finish()
        assert empty.n_pos == 0 and empty.sites().shape == (0, 12) and empty.columns().shape == (0, 8)
        empty.free()
    finally:
        p.free(); other.free()


# ---- the compressor's table ---------------------------------------------------------------------------------------------------------------
def test_compressor_makes_one_table_from_its_geometry(ctx):
    cmp_, arena, pseudo = compressor_with_pseudo_reads(ctx)
    ctx.set_pileup(True)
    try:
        cmp_.genome_geometry(SEQ_LEN, READ_LEN, OVERLAP)
        cmp_.refs_add(arena)
        cmp_.refs_finish()
        with pytest.raises(N.ColordHipError) as x:                                      # chunks are still to be coded
            cmp_.pileup()
        assert x.value.status == N.CL_E_INVALID and "after the last cl_compressor_encode" in str(x.value)
    finally:
        ctx.set_pileup(False)
        cmp_.free(); arena.free(); pseudo.free()
    cmp_, arena, pseudo = compressor_with_pseudo_reads(ctx)                           # the flag off: no table, nothing to hand out
    try:
        cmp_.genome_geometry(SEQ_LEN, READ_LEN, OVERLAP)
        cmp_.refs_add(arena)
        cmp_.refs_finish()
        with pytest.raises(N.ColordHipError) as x:
            cmp_.pileup()
        assert x.value.status == N.CL_E_INVALID and "no table" in str(x.value)
    finally:
        cmp_.free(); arena.free(); pseudo.free()


@pytest.mark.parametrize("what,text", [("geometry", "cl_ctx_set_pileup: needs the geometry of the pseudo reads"), ("pseudo", "cl_ctx_set_pileup: needs the pseudo reads of a reference genome")])
def test_pileup_without_pseudo_reads_or_geometry_is_refused(ctx, what, text):
    cmp_, arena, pseudo = compressor_with_pseudo_reads(ctx, with_pseudo=what == "geometry")
    ctx.set_pileup(True)
    try:
        cmp_.refs_add(arena)
        with pytest.raises(N.ColordHipError) as x:
            cmp_.refs_finish()
        assert x.value.status == N.CL_E_INVALID and text in str(x.value), str(x.value)
    finally:
        ctx.set_pileup(False)
        cmp_.free(); arena.free()
        if pseudo is not None:
            pseudo.free()


def test_one_shard_refuses_the_flag(ctx):
    from test_gpu_stream import one_call
    g = golden("s6m_ont")
    ctx.set_pileup(True)
    try:
        with pytest.raises(N.ColordHipError) as x:
            one_call(ctx, g.reads, params_of(g), [int(v) for v in g.reads.pack_bounds()], None)
        assert x.value.status == N.CL_E_UNSUPPORTED and "cl_ctx_set_pileup" in str(x.value)
    finally:
        ctx.set_pileup(False)
