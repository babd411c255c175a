"""GPU suite of the edit-operation profile (csrc/edits.hip): k_edit_profile against tests/edits_ref.py — on the streams tapped from
the unmodified reference (golden es.bin), on the hand-made streams of tests/editstreams.py (the window's edge, runs across it, the bins' edges, the
alternative table full) with the default launch, with a flush after every quad and with one block; malformed streams that stay inside every buffer;
and in the pipeline: cl_compress_shard and the chunked compressor (encode lanes included) with cl_ctx_set_edit_profile."""
import ctypes as C
import numpy as np
import pytest
import torch
from util import golden
from colord_amd import _native as N
from colord_amd.fastq import ReadSet
import edits_ref as E
import editstreams as ES
from test_edits_cpu import golden_refs, judged
from test_gpu_stream import params_of, one_call, chunked
from test_gpu_encode import sparse_g

pytestmark = pytest.mark.gpu

TAPPED = ["c1_ont_default", "c2_hifi_org", "c3_clr_ratio", "c7_hifi_balanced", "s3m_ont_n_ratio", "s5m_hifi", "s4m_ont_k23_balanced"]     # those of tests/test_gpu_expand.py


def readset_of(seqs):
    lens = np.array([len(s) for s in seqs], np.int64)
    return ReadSet(np.concatenate([np.asarray(s, np.uint8) for s in seqs]), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), None, [], [], False)


def to_device(streams, device):
    raw = np.frombuffer(b"".join(streams), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    return torch.from_numpy(raw).to(device), torch.from_numpy(off).to(device)


# ---- 1. the reference's own streams -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", TAPPED)
def test_kernel_equals_the_reference_on_tapped_streams(ctx, cfg):
    refs = ctx.pack_readset(readset_of(golden_refs(cfg)))
    es, off = to_device([e[2] for e in golden(cfg).es], ctx.device)
    got = ctx.edit_profile_of(refs, es, off).as_dict()
    refs.free()
    assert E.same(got, judged(cfg)) is None, E.same(got, judged(cfg))
    assert E.invariants(got) == []


# ---- 2. + 3. hand-made streams --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand(ctx):
    ref_seqs = ES.references()
    S = ES.hand_made()
    names, streams = list(S), list(S.values())
    per = [E.profile_of_read(s, ref_seqs, i) for i, s in enumerate(streams)]
    refs = ctx.pack_readset(readset_of(ref_seqs))
    yield refs, names, streams, per, E.profile(streams, ref_seqs)
    refs.free()


def test_hand_made_streams_one_by_one(ctx, hand):
    """each stream alone, so that a difference names the stream (a read per call: the other three waves of the block are idle)"""
    refs, names, streams, per, _ = hand
    bad = []
    for name, s, want in zip(names, streams, per):
        es, off = to_device([s], ctx.device)
        got = ctx.edit_profile_of(refs, es, off).as_dict()
        if E.same(got, want) is not None:
            bad.append((name, E.same(got, want)))
    assert not bad, bad


@pytest.mark.parametrize("flush_bytes,max_blocks", [(0, 0), (64, 0), (0, 1), (1, 2)], ids=["defaults", "flush_64", "one_block", "flush_1_two_blocks"])
def test_hand_made_set_with_every_launch_shape(ctx, hand, flush_bytes, max_blocks):
    refs, _, streams, _, want = hand
    es, off = to_device(streams, ctx.device)
    got = ctx.edit_profile_of(refs, es, off, flush_bytes, max_blocks).as_dict()
    assert E.same(got, want) is None, E.same(got, want)
    acc = ctx.edit_profile_of(refs, es, off, flush_bytes, max_blocks)           # a second batch into the same total
    acc = ctx.edit_profile_of(refs, es, off, flush_bytes, max_blocks, acc)
    assert E.same(acc.as_dict(), E.add(want, want)) is None


def test_no_reads_is_nothing(ctx, hand):
    refs = hand[0]
    got = ctx.edit_profile_of(refs, torch.zeros(0, dtype=torch.uint8, device=ctx.device), torch.zeros(1, dtype=torch.int64, device=ctx.device))
    assert bytes(got) == bytes(8 * E.WORDS)


# ---- 4. malformed, yet inside every buffer --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ES.malformed_device()))
def test_malformed_stream_is_refused_and_nothing_is_added(ctx, hand, name):
    refs, _, streams, _, _ = hand
    bad, why = ES.malformed_device()[name]
    good = [streams[3], streams[40], streams[41], streams[-2], streams[-1]]
    acc = ctx.edit_profile_of(refs, *to_device(good, ctx.device))
    before = bytes(acc)
    es, off = to_device(good[:4] + [bad] + good[4:], ctx.device)
    with pytest.raises(N.ColordHipError) as x:
        ctx.edit_profile_of(refs, es, off, acc=acc)
    assert x.value.status == N.CL_E_INVALID and "read 4: " + why in str(x.value), str(x.value)
    assert bytes(acc) == before


# ---- 5. the pipeline ------------------------------------------------------------------------------------------------------------------
def chunked_with_accessor(ctx, rs, prm, packs, cuts, announce):
    """the chunk loop of tests/test_gpu_stream.py (no quality stream), asking the COMPRESSOR for the profile before it is freed"""
    off, chunks = rs.offsets, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        r0, r1 = int(packs[a]), int(packs[b])
        o = torch.from_numpy((off[r0:r1 + 1] - off[r0]).astype(np.int64))
        chunks.append((ctx.pack_reads(torch.from_numpy(rs.bases[off[r0]:off[r1]]), o), (np.asarray(packs[a:b + 1]) - packs[a]).astype(np.uint32), o.to(ctx.device)))
    cmp_ = ctx.compressor(prm, None, None, None, expected_bases=int(off[-1]))
    for arena, *_ in chunks:
        cmp_.count_add(arena)
    cmp_.count_finish()
    for arena, *_ in chunks:
        cmp_.refs_add(arena)
    cmp_.refs_finish()
    if announce:
        for arena, pb, _ in chunks:
            cmp_.prepare(arena, pb)
    dna = b""
    for arena, pb, o in chunks:
        d, *_ = cmp_.encode(arena, pb, pb, None, o)
        dna += d.cpu().numpy().tobytes()
    prof = cmp_.edit_profile().as_dict()
    cmp_.free()
    for arena, *_ in chunks:
        arena.free()
    return dna, prof


@pytest.mark.parametrize("cfg", ["s6m_ont", "s5m_hifi"])
def test_drivers_profile_and_write_the_same_parts(ctx, cfg):
    """with the reference's parameters and packs (those of test_compress_shard_one_call_equals_reference: the tuple streams are the reference's, byte
    for byte): two chunks, one per pack, announced to the encode lanes; and one chunk on the caller's context"""
    g = golden(cfg)
    rs = g.reads
    prm = dict(params_of(g), sparse_g=sparse_g(g))
    packs = [int(x) for x in rs.pack_bounds()]
    assert len(packs) == 3
    cuts = [0, 1, 2]
    want = judged(cfg)
    never_one = one_call(ctx, rs, prm, packs, None)
    never_chunked = chunked(ctx, rs, prm, packs, cuts, None, announce="all")
    assert bytes(ctx.edit_profile()) == bytes(8 * E.WORDS), "a profile was counted although the flag was never set"
    ctx.set_edit_profile(True)
    try:
        on_one = one_call(ctx, rs, prm, packs, None)
        got_one = ctx.edit_profile().as_dict()
        ctx.set_edit_profile(False); ctx.set_edit_profile(True)                 # (switching it on clears the total, the lanes' included)
        on_chunked = chunked(ctx, rs, prm, packs, cuts, None, announce="all")  # stage A on the encode lanes
        got_lanes = ctx.edit_profile().as_dict()
        ctx.set_edit_profile(False); ctx.set_edit_profile(True)
        dna_own, got_own = chunked_with_accessor(ctx, rs, prm, packs, [0, 2], announce=False)   # stage A on the caller's context
    finally:
        ctx.set_edit_profile(False)
    assert on_one[:4] == never_one[:4], "one-call driver: parts differ with the profile on"
    assert on_chunked[:4] == never_chunked[:4], "chunked compressor: parts differ with the profile on"
    assert dna_own == never_chunked[0]
    for got, who in ((got_one, "one call"), (got_lanes, "lanes"), (got_own, "own context")):
        assert E.same(got, want) is None, (who, E.same(got, want))
    ctx.set_edit_profile(True)                                                  # (a fresh, empty total for whoever uses the context next)
    ctx.set_edit_profile(False)
    assert bytes(ctx.edit_profile()) == bytes(8 * E.WORDS)
