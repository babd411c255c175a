"""GPU suite of the lift of the read-to-genome mappings (csrc/mappings.hip): k_map_lift against its host twin (cl_mappings_lift_host)
and against tests/mappings_ref.py, record for record, on the constructed geometries and records of tests/mappingcases.py — no record, one, a wave,
a wave and one, more than a block, more than the grid's first stride; all dropped, none, alternating (stable order); the capacity protocol; the
three refused records; and the geometry a compressor is given behind its pseudo reads, with the refusals of cl_ctx_set_mappings."""
import ctypes as C
import numpy as np
import pytest
import torch
from util import golden
from colord_amd import _native as N
import mappings_ref as MR
import mappingcases as MC
from test_mappings_cpu import host_lift
from test_gpu_stream import params_of

pytestmark = pytest.mark.gpu


def to_device(recs, ctx):
    return torch.from_numpy(np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, 12).view(np.int32)).to(ctx.device)


def records_of(t):
    return t.cpu().numpy().view(np.uint32).reshape(-1, 12)


@pytest.mark.parametrize("geo", sorted(MC.GEOMETRIES))
@pytest.mark.parametrize("mode", MC.MODES)
def test_kernel_equals_the_host_twin_and_the_judge(ctx, geo, mode):
    G = MC.GEOMETRIES[geo]
    for n in MC.SIZES:
        recs = MC.records(G, n, mode)
        want = MR.lift(recs, **G)
        st, host, m, _, _ = host_lift(recs, G)
        got = records_of(ctx.mappings_lift(to_device(recs, ctx), G["seq_len"], G["read_len"], G["overlap"]))
        assert st == 0 and m == len(want) and np.array_equal(host, want), (geo, mode, n)
        assert got.shape == want.shape and np.array_equal(got, want), (geo, mode, n)


def test_capacity_protocol(ctx):
    """too little room: the need is reported and nothing is written; exactly enough: the records, and the one behind them stays"""
    G = MC.NINE
    recs = MC.records(G, 257, "alternating")
    want = MR.lift(recs, **G)
    d, sl, need = to_device(recs, ctx), np.asarray(G["seq_len"], np.uint64), C.c_uint64(0)
    out = torch.full((len(want) + 1, 12), 0x5a5a5a5a, dtype=torch.int32, device=ctx.device)
    for cap in (0, 1, len(want) - 1):
        st = ctx.lib.cl_mappings_lift(ctx.h, d.data_ptr(), len(recs), sl.ctypes.data, len(sl), G["read_len"], G["overlap"], out.data_ptr(), cap, C.byref(need))
        torch.cuda.synchronize()
        assert st == N.CL_E_CAPACITY and need.value == len(want) and bool((out == 0x5a5a5a5a).all())
    with pytest.raises(N.ColordHipError) as x:
        ctx.mappings_lift(d, G["seq_len"], G["read_len"], G["overlap"], cap=len(want) - 1)
    assert x.value.status == N.CL_E_CAPACITY and "need %d records" % len(want) in str(x.value)
    st = ctx.lib.cl_mappings_lift(ctx.h, d.data_ptr(), len(recs), sl.ctypes.data, len(sl), G["read_len"], G["overlap"], out.data_ptr(), len(want), C.byref(need))
    torch.cuda.synchronize()
    assert st == N.CL_OK and need.value == len(want)
    assert np.array_equal(records_of(out[:len(want)]), want) and bool((out[len(want)] == 0x5a5a5a5a).all())


@pytest.mark.parametrize("name", ["tlen", "position", "end"])
def test_a_record_that_cannot_be_lifted_is_refused_and_nothing_is_handed_out(ctx, name):
    G = MC.NINE
    recs, first, code = MC.refused()[name]
    d = to_device(recs, ctx)
    with pytest.raises(N.ColordHipError) as x:
        ctx.mappings_lift(d, G["seq_len"], G["read_len"], G["overlap"])
    assert x.value.status == N.CL_E_INVALID and "record %d: " % first in str(x.value), str(x.value)
    st, _, n, bad, c = host_lift(recs, G)
    assert (st, n, bad, c) == (N.CL_E_INVALID, 0, first, code)
    sl, need = np.asarray(G["seq_len"], np.uint64), C.c_uint64(77)
    out = torch.full((len(recs), 12), 0x5a5a5a5a, dtype=torch.int32, device=ctx.device)
    st = ctx.lib.cl_mappings_lift(ctx.h, d.data_ptr(), len(recs), sl.ctypes.data, len(sl), G["read_len"], G["overlap"], out.data_ptr(), len(recs), C.byref(need))
    torch.cuda.synchronize()
    assert st == N.CL_E_INVALID and need.value == 0 and bool((out == 0x5a5a5a5a).all())


def test_refused_geometries_of_the_lift(ctx):
    d = to_device(MC.records(MC.ONE, 3, "none_dropped"), ctx)
    for seq_len, read_len, overlap, status in (([1000], 50, 50, N.CL_E_INVALID), ([1000], 10, 50, N.CL_E_INVALID), ([1 << 32], 300, 50, N.CL_E_UNSUPPORTED)):
        with pytest.raises(N.ColordHipError) as x:
            ctx.mappings_lift(d, seq_len, read_len, overlap)
        assert x.value.status == status
    assert ctx.mappings_lift(d, [], 300, 50).shape == (0, 12)                          # no sequence: every record names a read


# ---- the geometry of a compressor's pseudo reads ------------------------------------------------------------------------------------------
SEQ_LEN, READ_LEN, OVERLAP = [5000, 1200, 700], 2000, 190


def compressor_with_pseudo_reads(ctx, with_pseudo=True):
    """the reads of a golden through pass 1, then the pieces of a random three-sequence genome as pseudo reads"""
    g = golden("s6m_ont")
    rs = g.reads
    arena = ctx.pack_readset(rs)
    cmp_ = ctx.compressor(params_of(g), None, None, None, expected_bases=int(rs.offsets[-1]))
    cmp_.count_add(arena)
    cmp_.count_finish()
    pseudo = None
    if with_pseudo:
        rng = np.random.default_rng(8)
        seqs = [rng.integers(0, 4, ln, dtype=np.uint8) for ln in SEQ_LEN]
        P = [seqs[s][a:a + ln] for s, a, ln in MR.pieces(SEQ_LEN, READ_LEN, OVERLAP)]
        pseudo = ctx.pack_reads(torch.from_numpy(np.concatenate(P)), torch.from_numpy(np.cumsum([0] + [len(p) for p in P]).astype(np.int64)))
        cmp_.pseudo_reads(pseudo)
    return cmp_, arena, pseudo


def test_compressor_takes_the_geometry_of_its_pseudo_reads_and_no_other(ctx):
    assert len(MR.pieces(SEQ_LEN, READ_LEN, OVERLAP)) == 3 + 1 + 1
    cmp_, arena, pseudo = compressor_with_pseudo_reads(ctx)
    try:
        for seq_len, read_len, overlap, status, text in (
                (SEQ_LEN, 1000, OVERLAP, N.CL_E_INVALID, "pieces"),                         # another piece count
                ([5000, 1200, 701], READ_LEN, OVERLAP, N.CL_E_INVALID, "pseudo read 4 has 700 bases"),      # the same count, another length
                ([5000, 1200], READ_LEN, OVERLAP, N.CL_E_INVALID, "pieces"),
                ([1200, 5000, 700], READ_LEN, OVERLAP, N.CL_E_INVALID, "pseudo read"),      # the same lengths in another order
                (SEQ_LEN, 190, 190, N.CL_E_INVALID, "exceed the overlap"),
                ([1 << 32], READ_LEN, OVERLAP, N.CL_E_UNSUPPORTED, "2^32")):
            with pytest.raises(N.ColordHipError) as x:
                cmp_.genome_geometry(seq_len, read_len, overlap)
            assert x.value.status == status and text in str(x.value), str(x.value)
        cmp_.genome_geometry(SEQ_LEN, READ_LEN, OVERLAP)
        with pytest.raises(N.ColordHipError) as x:                                          # once
            cmp_.genome_geometry(SEQ_LEN, READ_LEN, OVERLAP)
        assert x.value.status == N.CL_E_INVALID
        ctx.set_mappings(True)
        cmp_.refs_add(arena)
        cmp_.refs_finish()                                                                  # pseudo reads and their geometry: accepted
        assert cmp_.mappings().shape == (0, 12) and ctx.mappings().shape == (0, 12)
    finally:
        ctx.set_mappings(False)
        cmp_.free(); arena.free(); pseudo.free()


@pytest.mark.parametrize("what,text", [("geometry", "needs the geometry of the pseudo reads"), ("pseudo", "needs the pseudo reads of a reference genome")])
def test_mappings_without_pseudo_reads_or_geometry_are_refused(ctx, what, text):
    cmp_, arena, pseudo = compressor_with_pseudo_reads(ctx, with_pseudo=what == "geometry")
    ctx.set_mappings(True)
    try:
        cmp_.refs_add(arena)
        with pytest.raises(N.ColordHipError) as x:
            cmp_.refs_finish()
        assert x.value.status == N.CL_E_INVALID and text in str(x.value), str(x.value)
    finally:
        ctx.set_mappings(False)
        cmp_.free(); arena.free()
        if pseudo is not None:
            pseudo.free()


def test_one_shard_refuses_the_flag(ctx):
    from test_gpu_stream import one_call
    g = golden("s6m_ont")
    ctx.set_mappings(True)
    try:
        with pytest.raises(N.ColordHipError) as x:
            one_call(ctx, g.reads, params_of(g), [int(v) for v in g.reads.pack_bounds()], None)
        assert x.value.status == N.CL_E_UNSUPPORTED and "cl_ctx_set_mappings" in str(x.value)
    finally:
        ctx.set_mappings(False)
