"""GPU suite of the CIGARs (csrc/cigars.hip): k_cigar_walk against its host twin (cl_cigars_host) and against tests/cigars_ref.py,
counts and operations — on the hand-made streams of tests/editstreams.py, tests/overlapstreams.py and tests/cigarstreams.py one by one and as sets
(default launch, one block; with and without a limit on the reference ids), the capacity protocol, no reads, malformed streams that stay inside
every buffer, and on the streams the encoder makes of a small synthetic set, with the relations holding against cl_overlaps_of's records."""
import ctypes as C
import numpy as np
import pytest
import torch
from util import golden
from colord_amd import _native as N
import cigars_ref as CR
import cigarstreams as CS
import editstreams as ES
import overlapstreams as OS
from test_cigars_cpu import host_cigars
from test_edits_cpu import golden_refs
from test_gpu_edits import readset_of, to_device

pytestmark = pytest.mark.gpu
FILL = 0x5a5a5a5a


def words_of(t):
    return t.cpu().numpy().view(np.uint32)


def device_cigars(ctx, refs, streams, id_limit=0, max_blocks=0):
    es, off = to_device(streams, ctx.device)
    rec, ops = ctx.cigars_of(refs, es, off, id_limit, max_blocks)
    return words_of(rec), words_of(ops)


@pytest.fixture(scope="module")
def hand(ctx):
    ref_seqs = ES.references()
    S = {**ES.hand_made(), **OS.hand_made(), **CS.hand_made()}
    refs = ctx.pack_readset(readset_of(ref_seqs))
    yield refs, list(S), list(S.values()), ref_seqs
    refs.free()


@pytest.fixture(scope="module")
def read_set():
    """the judge over the read set, computed once: (streams, without a limit, with the limit in the middle of the ids)"""
    streams, ref_seqs = CS.read_set(), ES.references()
    return streams, CR.cigars(streams, ref_seqs), CR.cigars(streams, ref_seqs, CS.ID_LIMIT)


def test_hand_made_streams_one_by_one(ctx, hand):
    """each stream alone, so that a difference names the stream: kernel == host twin == judge, counts and operations"""
    refs, names, streams, ref_seqs = hand
    bad = []
    for name, s in zip(names, streams):
        want_rec, want_ops = CR.cigars([s], ref_seqs)
        st, host_rec, host_ops, _, _, _ = host_cigars([s], ref_seqs)
        rec, ops = device_cigars(ctx, refs, [s])
        if st != 0 or not (np.array_equal(rec, want_rec) and np.array_equal(ops, want_ops) and np.array_equal(host_rec, want_rec) and np.array_equal(host_ops, want_ops)):
            bad.append((name, rec.tolist(), want_rec.tolist(), [CR.text(cg) for cg in CR.split(rec, ops)] if rec.sum() == len(ops) else ops.tolist(), [CR.text(cg) for cg in CR.split(want_rec, want_ops)]))
    assert not bad, bad[:3]


@pytest.mark.parametrize("id_limit", [0, CS.ID_LIMIT], ids=["every_id", "limit"])
def test_read_set_with_one_block_and_the_default_grid(ctx, hand, read_set, id_limit):
    """plain reads, script reads with 0, 1 and 66 records, a record of one operation next to one of 301: a record's place comes from the scan over the
    reads, its operations' place from the scan over the records; max_blocks = 1 and the default grid give the same bytes"""
    refs, _, _, ref_seqs = hand
    streams, every, limited = read_set
    want_rec, want_ops = limited if id_limit else every
    st, host_rec, host_ops, _, _, _ = host_cigars(streams, ref_seqs, id_limit)
    assert st == 0 and np.array_equal(host_rec, want_rec) and np.array_equal(host_ops, want_ops)
    got = [device_cigars(ctx, refs, streams, id_limit, mb) for mb in (0, 1)]
    for rec, ops in got:
        assert np.array_equal(rec, want_rec) and np.array_equal(ops, want_ops)
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    recs = ctx.overlaps_of(refs, *to_device(streams, ctx.device)).cpu().numpy().view(np.uint32).reshape(-1, 12)
    assert CR.invariants(recs, got[0][0], got[0][1], zero_ok=bool(id_limit)) == []
    if id_limit:
        assert np.array_equal(got[0][0] == 0, recs[:, 1] >= id_limit)


def test_all_hand_made_streams_at_once(ctx, hand):
    refs, _, streams, ref_seqs = hand
    want_rec, want_ops = CR.cigars(streams, ref_seqs)
    for mb in (0, 1):
        rec, ops = device_cigars(ctx, refs, streams, 0, mb)
        assert np.array_equal(rec, want_rec) and np.array_equal(ops, want_ops)


def test_capacity_protocol(ctx, hand, read_set):
    """too little room for either: both needs are reported and nothing is written; exactly enough: the words, and the one behind them stays"""
    refs = hand[0]
    streams, (want_rec, want_ops), _ = read_set
    es, off = to_device(streams, ctx.device)
    nr, no = C.c_uint64(0), C.c_uint64(0)
    rec = torch.full((len(want_rec) + 1,), FILL, dtype=torch.int32, device=ctx.device)
    ops = torch.full((len(want_ops) + 1,), FILL, dtype=torch.int32, device=ctx.device)
    call = lambda rc, oc: ctx.lib.cl_cigars_of(ctx.h, refs.h, es.data_ptr(), off.data_ptr(), len(streams), 0, 0, rec.data_ptr(), rc, C.byref(nr), ops.data_ptr(), oc, C.byref(no))
    for rc, oc in ((0, 0), (len(want_rec) - 1, len(want_ops)), (len(want_rec), len(want_ops) - 1), (len(want_rec), 0)):
        st = call(rc, oc)
        torch.cuda.synchronize()
        assert st == N.CL_E_CAPACITY and (nr.value, no.value) == (len(want_rec), len(want_ops)) and bool((rec == FILL).all()) and bool((ops == FILL).all())
    with pytest.raises(N.ColordHipError) as x:
        ctx.cigars_of(refs, es, off, caps=(len(want_rec), len(want_ops) - 1))
    assert x.value.status == N.CL_E_CAPACITY and "need %d records and %d operations" % (len(want_rec), len(want_ops)) in str(x.value)
    st = call(len(want_rec), len(want_ops))
    torch.cuda.synchronize()
    assert st == N.CL_OK and (nr.value, no.value) == (len(want_rec), len(want_ops))
    assert np.array_equal(words_of(rec[:-1]), want_rec) and np.array_equal(words_of(ops[:-1]), want_ops) and int(rec[-1]) == FILL and int(ops[-1]) == FILL


def test_no_reads_and_no_records_are_nothing(ctx, hand):
    refs, _, streams, _ = hand
    rec, ops = ctx.cigars_of(refs, torch.zeros(0, dtype=torch.uint8, device=ctx.device), torch.zeros(1, dtype=torch.int64, device=ctx.device))
    assert rec.numel() == 0 and ops.numel() == 0
    plain = [s for s in streams if s[0] >> 4 != ES.START_ES]                     # plain reads only: reads, but no record
    rec, ops = device_cigars(ctx, refs, plain)
    assert len(plain) >= 4 and len(rec) == 0 and len(ops) == 0
    rec, ops = device_cigars(ctx, refs, streams, id_limit=0xffffffff)           # (a limit past every id is no limit)
    assert len(rec) > 100 and rec.min() >= 1 and len(ops) == int(rec.sum())


@pytest.mark.parametrize("name", sorted(ES.malformed_device()))
def test_malformed_stream_is_refused_with_the_hosts_read_and_code(ctx, hand, name):
    refs, _, streams, ref_seqs = hand
    bad, why = ES.malformed_device()[name]
    good = [streams[3], streams[40], streams[41], streams[-2], streams[-1]]
    sset = good[:4] + [bad] + good[4:]
    st, _, _, need, read, text = host_cigars(sset, ref_seqs)
    assert (st, need, read, text) == (N.CL_E_INVALID, (0, 0), 4, why)
    es, off = to_device(sset, ctx.device)
    with pytest.raises(N.ColordHipError) as x:
        ctx.cigars_of(refs, es, off)
    assert x.value.status == N.CL_E_INVALID and "read %d: %s" % (read, text) in str(x.value), str(x.value)
    nr, no = C.c_uint64(77), C.c_uint64(77)
    rec = torch.full((4096,), FILL, dtype=torch.int32, device=ctx.device)
    ops = torch.full((65536,), FILL, dtype=torch.int32, device=ctx.device)
    st = ctx.lib.cl_cigars_of(ctx.h, refs.h, es.data_ptr(), off.data_ptr(), 6, 0, 0, rec.data_ptr(), 4096, C.byref(nr), ops.data_ptr(), 65536, C.byref(no))
    torch.cuda.synchronize()
    assert st == N.CL_E_INVALID and (nr.value, no.value) == (0, 0) and bool((rec == FILL).all()) and bool((ops == FILL).all())


def test_encoder_made_streams(ctx):
    """s6m_ont, a synthetic set (374 reads of a 200-kb genome): the streams cl_encode_reads makes of it — kernel == host twin, and every record of
    cl_overlaps_of with its operations"""
    from test_gpu_encode import gpu_streams
    from test_gpu_dna import ref_subset
    g = golden("s6m_ont")
    es, off, _ = gpu_streams(ctx, g)
    streams = [es[off[i]:off[i + 1]].tobytes() for i in range(g.reads.n_reads)]
    ref_seqs = golden_refs("s6m_ont")
    st, host_rec, host_ops, _, _, _ = host_cigars(streams, ref_seqs)
    assert st == 0 and len(host_rec) > 300 and len(host_ops) > 10 * len(host_rec)
    refs = ctx.pack_readset(ref_subset(g.reads, g.accept.astype(bool) & ~g.reads.has_n()))
    try:
        assert refs.n_reads == len(ref_seqs)
        d_es, d_off = torch.from_numpy(es).to(ctx.device), torch.from_numpy(off.astype(np.int64)).to(ctx.device)
        rec, ops = (words_of(t) for t in ctx.cigars_of(refs, d_es, d_off))
        recs = ctx.overlaps_of(refs, d_es, d_off).cpu().numpy().view(np.uint32).reshape(-1, 12)
    finally:
        refs.free()
    assert np.array_equal(rec, host_rec) and np.array_equal(ops, host_ops)
    assert CR.invariants(recs, rec, ops) == []
    w_rec, w_ops = CR.cigars(streams, ref_seqs)
    assert np.array_equal(rec, w_rec) and np.array_equal(ops, w_ops)
