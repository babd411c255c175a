"""GPU suite of the overlap records (csrc/overlaps.hip): k_overlap_walk against tests/overlaps_ref.py — on the streams tapped from the
unmodified reference (golden es.bin), on the hand-made streams of tests/editstreams.py and tests/overlapstreams.py one by one and as sets (default
launch, one block; with and without a translation table), the capacity protocol, no reads, malformed streams that stay inside every buffer; in the
pipeline: cl_compress_shard and the chunked compressor with encode lanes (cl_ctx_set_overlaps); and a truth test on reads whose place on a genome is
known."""
import numpy as np
import pytest
import torch
from util import golden
from colord_amd import _native as N
import edits_ref as E
import editstreams as ES
import overlaps_ref as OR
import overlapstreams as OS
from test_edits_cpu import golden_refs
from test_gpu_edits import TAPPED, readset_of, to_device
from test_gpu_stream import params_of, one_call, chunked
from test_gpu_encode import sparse_g

pytestmark = pytest.mark.gpu


def records_of(t):
    return t.cpu().numpy().view(np.uint32).reshape(-1, 12)


# ---- 1. the reference's own streams -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", TAPPED)
def test_kernel_equals_the_reference_on_tapped_streams(ctx, cfg):
    ref_seqs = golden_refs(cfg)
    streams = [e[2] for e in golden(cfg).es]
    table = np.arange(len(ref_seqs), dtype=np.uint32)[::-1].copy() + 9
    want = OR.records(streams, ref_seqs, 5, table)
    refs = ctx.pack_readset(readset_of(ref_seqs))
    es, off = to_device(streams, ctx.device)
    got = records_of(ctx.overlaps_of(refs, es, off, 5, torch.from_numpy(table.view(np.int32)).to(ctx.device)))
    refs.free()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert OR.invariants(got) == []


# ---- 2. hand-made streams -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand(ctx):
    ref_seqs = ES.references()
    S = {**ES.hand_made(), **OS.hand_made()}
    names, streams = list(S), list(S.values())
    per = [OR.records_of_read(s, ref_seqs)[0] for s in streams]
    refs = ctx.pack_readset(readset_of(ref_seqs))
    yield refs, names, streams, per, ref_seqs
    refs.free()


def test_hand_made_streams_one_by_one(ctx, hand):
    """each stream alone, so that a difference names the stream (a read per call: the other three waves of the block are idle)"""
    refs, names, streams, per, _ = hand
    bad = []
    for name, s, want in zip(names, streams, per):
        es, off = to_device([s], ctx.device)
        got = records_of(ctx.overlaps_of(refs, es, off))
        if got.tolist() != [list(w) for w in want]:
            bad.append((name, got.tolist(), want))
    assert not bad, bad[:3]


@pytest.mark.parametrize("max_blocks", [0, 1], ids=["defaults", "one_block"])
@pytest.mark.parametrize("with_table", [False, True], ids=["ids", "translated"])
def test_both_hand_made_sets_at_once(ctx, hand, max_blocks, with_table):
    """the hand-made streams and the read set whose reads give 0, 1 and 66 records in turn: every read's place comes from the scan"""
    refs, _, streams, _, ref_seqs = hand
    sset = OS.read_set() + streams + OS.read_set()
    table = (np.arange(len(ref_seqs), dtype=np.uint32) * 3 + 1) if with_table else None
    want = OR.records(sset, ref_seqs, 100, table)
    es, off = to_device(sset, ctx.device)
    got = records_of(ctx.overlaps_of(refs, es, off, 100, None if table is None else torch.from_numpy(table.view(np.int32)).to(ctx.device), max_blocks))
    assert got.shape == want.shape and np.array_equal(got, want)
    assert OR.invariants(got) == []


def test_capacity_protocol(ctx, hand):
    """too little room: the need is reported and nothing is written; exactly enough: the records"""
    refs, _, streams, _, ref_seqs = hand
    want = OR.records(streams, ref_seqs)
    es, off = to_device(streams, ctx.device)
    import ctypes as C
    need = C.c_uint64(0)
    out = torch.full((len(want) + 1, 12), 0x5a5a5a5a, dtype=torch.int32, device=ctx.device)
    for cap in (0, 1, len(want) - 1):
        st = ctx.lib.cl_overlaps_of(ctx.h, refs.h, es.data_ptr(), off.data_ptr(), len(streams), 0, None, 0, 0, out.data_ptr(), cap, C.byref(need))
        torch.cuda.synchronize()
        assert st == N.CL_E_CAPACITY and need.value == len(want) and bool((out == 0x5a5a5a5a).all())
    with pytest.raises(N.ColordHipError) as x:
        ctx.overlaps_of(refs, es, off, cap=len(want) - 1)
    assert x.value.status == N.CL_E_CAPACITY and "need %d records" % len(want) in str(x.value)
    st = ctx.lib.cl_overlaps_of(ctx.h, refs.h, es.data_ptr(), off.data_ptr(), len(streams), 0, None, 0, 0, out.data_ptr(), len(want), C.byref(need))
    torch.cuda.synchronize()
    assert st == N.CL_OK and need.value == len(want)
    assert np.array_equal(records_of(out[:len(want)]), want) and bool((out[len(want)] == 0x5a5a5a5a).all())       # (the record behind the last stays as it was)


def test_no_reads_is_nothing(ctx, hand):
    refs = hand[0]
    got = ctx.overlaps_of(refs, torch.zeros(0, dtype=torch.uint8, device=ctx.device), torch.zeros(1, dtype=torch.int64, device=ctx.device))
    assert got.shape == (0, 12)
    plain = [s for s in hand[2] if s[0] >> 4 != E.START_ES]                       # plain reads only: reads, but no record
    assert len(plain) >= 4 and ctx.overlaps_of(refs, *to_device(plain, ctx.device)).shape == (0, 12)


# ---- 3. malformed, yet inside every buffer --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ES.malformed_device()))
def test_malformed_stream_is_refused_and_nothing_is_handed_out(ctx, hand, name):
    import ctypes as C
    refs, _, streams, _, _ = hand
    bad, why = ES.malformed_device()[name]
    good = [streams[3], streams[40], streams[41], streams[-2], streams[-1]]
    es, off = to_device(good[:4] + [bad] + good[4:], ctx.device)
    with pytest.raises(N.ColordHipError) as x:
        ctx.overlaps_of(refs, es, off)
    assert x.value.status == N.CL_E_INVALID and "read 4: " + why in str(x.value), str(x.value)
    need = C.c_uint64(77)
    out = torch.full((4096, 12), 0x5a5a5a5a, dtype=torch.int32, device=ctx.device)
    st = ctx.lib.cl_overlaps_of(ctx.h, refs.h, es.data_ptr(), off.data_ptr(), 6, 0, None, 0, 0, out.data_ptr(), 4096, C.byref(need))
    torch.cuda.synchronize()
    assert st == N.CL_E_INVALID and need.value == 0 and bool((out == 0x5a5a5a5a).all())


# ---- 4. the pipeline ------------------------------------------------------------------------------------------------------------------
def test_drivers_keep_the_records_and_write_the_same_parts(ctx):
    """s6m_ont, a synthetic set (374 reads of a 200-kb genome) with the reference's parameters and packs, where the tuple streams are the
    reference's byte for byte (test_gpu_edits.py): the records must be the judge's walk over those streams, reference ids translated by the
    acceptor's decisions; two chunks on encode lanes must give those of one call; and no part may change."""
    g = golden("s6m_ont")
    rs = g.reads
    prm = dict(params_of(g), sparse_g=sparse_g(g))
    packs = [int(x) for x in rs.pack_bounds()]
    assert len(packs) == 3
    accepted = g.accept[len(g.accept) - rs.n_reads:].astype(bool) & ~rs.has_n()
    table = np.nonzero(accepted)[0].astype(np.uint32)                         # reference id -> index of that read in the input
    assert 0 < len(table) < rs.n_reads // 4                                     # (the sparse acceptor: a translation that is not the identity)
    want = OR.records([e[2] for e in g.es], golden_refs("s6m_ont"), 0, table)
    assert len(want) > 300 and OR.invariants(want) == [] and (want[:, 1] < want[:, 0]).all()        # (a read is coded against EARLIER reads)
    ctx.set_overlaps(True); ctx.set_overlaps(False)                             # (whatever a test before left on the shared context is dropped)
    never_one = one_call(ctx, rs, prm, packs, None)
    never_chunked = chunked(ctx, rs, prm, packs, [0, 1, 2], None, announce="all")
    assert ctx.overlaps().shape == (0, 12), "records were kept although the flag was never set"
    ctx.set_overlaps(True)
    try:
        on_one = one_call(ctx, rs, prm, packs, None)
        got_one = ctx.overlaps()
        ctx.set_overlaps(False); ctx.set_overlaps(True)                         # (switching it on drops what was kept, the lanes' included)
        on_chunked = chunked(ctx, rs, prm, packs, [0, 1, 2], None, announce="all")    # stage A on the encode lanes
        got_lanes = ctx.overlaps()
    finally:
        ctx.set_overlaps(False)
    assert on_one[:4] == never_one[:4], "one-call driver: parts differ with the option on"
    assert on_chunked[:4] == never_chunked[:4], "chunked compressor: parts differ with the option on"
    for got, who in ((got_one, "one call"), (got_lanes, "lanes")):
        assert got.shape == want.shape and np.array_equal(got, want), who
    ctx.set_overlaps(True)                                                      # (a fresh, empty list for whoever uses the context next)
    ctx.set_overlaps(False)
    assert ctx.overlaps().shape == (0, 12)


# ---- 5. truth -------------------------------------------------------------------------------------------------------------------------
def reads_with_coordinates(seed=20, genome_len=200_000, n_reads=60, err=(0.02, 0.03, 0.02)):
    """about 60 reads of 2 - 5 kb from either strand of a random genome with the ONT error rates of colord_amd/synth.py (deletion, substitution,
    insertion per base) -> (sequences, per read the genome coordinate of every base, strands); an inserted base takes its left neighbour's
    coordinate (the first base's when it is the first)"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, genome_len, dtype=np.uint8)
    e_del, e_sub, e_ins = err
    seqs, coords, strands = [], [], []
    for _ in range(n_reads):
        ln = int(rng.integers(2000, 5001))
        st = int(rng.integers(0, genome_len - ln))
        s, c = genome[st:st + ln].copy(), np.arange(st, st + ln)
        rev = bool(rng.random() < 0.5)
        if rev:
            s, c = (3 - s[::-1]).astype(np.uint8), c[::-1].copy()
        r = rng.random(ln)
        sub = (r >= e_del) & (r < e_del + e_sub)
        s[sub] = (s[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
        s, c = s[r >= e_del], c[r >= e_del]
        ins = np.nonzero(rng.random(len(s)) < e_ins)[0]
        s = np.insert(s, ins, rng.integers(0, 4, len(ins)).astype(np.uint8))
        c = np.insert(c, ins, c[np.maximum(ins - 1, 0)])
        seqs.append(s.astype(np.uint8)); coords.append(c); strands.append(rev)
    return seqs, coords, strands


def test_records_lie_where_the_reads_come_from(ctx):
    """Every read is a reference read (-R all), k-mers kept from two occurrences on, a candidate from 2 % of shared m-mers on: at a coverage of one,
    overlaps are partial.  For every record with anchor bases the genome interval of q[qs:qe] and that of t[ts:te] must intersect and the strand
    flag must be the true relative strand; at least half of the reads coded by script must yield a record.  No tolerance: an anchor is an exact
    16-mer match, and a random 200-kb genome repeats no 16-mer by chance often enough to place a read elsewhere."""
    seqs, coords, strands = reads_with_coordinates()
    rs = readset_of(seqs)
    prm = dict(params_of(golden("s6m_ont")), ci=2, f=4, sparse=0, frac_min=0.02)
    ctx.set_overlaps(True); ctx.set_edit_profile(True)
    try:
        one_call(ctx, rs, prm, [0, len(seqs)], None)
        recs, prof = ctx.overlaps(), ctx.edit_profile().as_dict()
    finally:
        ctx.set_overlaps(False); ctx.set_edit_profile(False)
    ctx.set_overlaps(True); ctx.set_overlaps(False)                             # (nothing is left on the shared context)
    n_script = int(prof["kind_reads"][2])
    f = {k: recs[:, i].astype(np.int64) for i, k in enumerate(OR.FIELDS)}
    print("script reads %d, records %d, with anchors %d, reads with a record %d" % (n_script, len(recs), int((f["anchor_bases"] > 0).sum()), len(set(f["q"].tolist()))))
    assert OR.invariants(recs) == [] and (f["t"] < f["q"]).all()
    assert (f["qlen"] == np.array([len(seqs[q]) for q in f["q"]])).all() and (f["tlen"] == np.array([len(seqs[t]) for t in f["t"]])).all()
    bad = []
    for i in np.nonzero(f["anchor_bases"] > 0)[0]:
        q, t = int(f["q"][i]), int(f["t"][i])
        cq, ct = coords[q][f["qs"][i]:f["qe"][i]], coords[t][f["ts"][i]:f["te"][i]]
        meet = max(cq.min(), ct.min()) <= min(cq.max(), ct.max())
        if not meet or bool(f["flags"][i] & OR.REV) != (strands[q] != strands[t]):
            bad.append((recs[i].tolist(), int(cq.min()), int(cq.max()), int(ct.min()), int(ct.max()), strands[q], strands[t]))
    assert not bad, bad[:5]
    assert n_script >= 1 and 2 * len(set(f["q"].tolist())) >= n_script
    assert int((f["anchor_bases"] > 0).sum()) >= 1
