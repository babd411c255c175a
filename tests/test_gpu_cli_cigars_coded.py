"""GPU suite of `colord_hip compress-* -G genome.fa --mappings --cigars --cigars-coded`: the `hipcigars` stream is version 2, its operations
coded on the device.  The input, the genome and the options are those of the truth test of tests/test_gpu_cli_cigars.py (60 reads of 2 - 5 kb on a
three-sequence genome), whose CIGARs walk their reads over the genome exactly: here the texts `info` prints from the coded archive must be those it
prints from the archive written with --cigars alone — that truth test at one remove."""
import os
import numpy as np
import pytest
from colord_amd import archive as AR, device as D
import cigarcoder_ref as CC
import cigars_ref as CR
import mappings_ref as MR
from test_gpu_cli_cigars import truth, inputs, run, streams, stored, SENSITIVE, SEQ_LEN      # noqa: F401 (truth and inputs are fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def archives(tmp_path_factory, inputs):
    fa, fq = inputs
    d = tmp_path_factory.mktemp("cgc_arc")
    raw, coded = str(d / "cigars.colord"), str(d / "coded.colord")
    run(["compress-ont", "-G", fa, "--mappings", "--cigars"] + SENSITIVE + [fq, raw])
    run(["compress-ont", "-G", fa, "--mappings", "--cigars", "--cigars-coded"] + SENSITIVE + [fq, coded])
    return raw, coded


def stored_coded(arc):
    """(records, counts, segment bytes, operations, segments) of a version-2 stream"""
    a = AR.read_archive(arc)
    assert len(a["hipcigars"].parts) == 1
    _, _, _, _, recs = MR.parse(a["hipmappings"].parts[0][1])
    b = a["hipcigars"].parts[0][1]
    version, op_bytes = np.frombuffer(b[:8], "<u4").tolist()
    nr, no, ns, nb = np.frombuffer(b[8:40], "<u8").tolist()
    assert (version, op_bytes) == (2, 4) and len(b) == 40 + 4 * nr + nb
    return recs, np.frombuffer(b[40:40 + 4 * nr], "<u4").copy(), b[40 + 4 * nr:], no, ns


def every_segment_is_the_host_twins(seg, ops):
    """a segment is coded on its own: each must be the host twin's bytes of its operations, however the batches fell; returns their number"""
    at = 0
    parts = CC.split_segments(seg)
    for n, b in parts:
        assert b == D.cigars_pack_host(ops[at:at + n])
        at += n
    assert at == len(ops) and b"".join(b for _, b in parts) == seg
    return len(parts)


def test_info_prints_the_same_texts_from_either_version(archives):
    raw, coded = archives
    for form in ("--cigar", "--sam"):
        a, b = run(["info", "--mappings", form, raw]).stdout, run(["info", "--mappings", form, coded]).stdout
        assert a == b and len(a.splitlines()) > 30
    assert run(["info", "--mappings", "--cigar", "--names", raw]).stdout == run(["info", "--mappings", "--cigar", "--names", coded]).stdout


def test_the_segments_decode_to_the_operations_of_version_1(archives):
    raw, coded = archives
    recs, rec_ops, ops = stored(raw)
    crecs, crec_ops, seg, no, ns = stored_coded(coded)
    assert np.array_equal(crecs, recs) and np.array_equal(crec_ops, rec_ops) and no == len(ops)
    assert np.array_equal(D.cigars_unpack_host(seg), ops) and np.array_equal(CC.unpack(seg), ops)
    assert every_segment_is_the_host_twins(seg, ops) == ns >= 1
    assert b"".join(CC.pack(list(ops[a:a + n])) for a, n in zip(np.cumsum([0] + [n for n, _ in CC.split_segments(seg)]), [n for n, _ in CC.split_segments(seg)])) == seg      # ... and the judge's
    n_esc = int((ops >> 4 > 255).sum())
    line = "cigars: %d operations of %d mapping records, coded: %d bytes in %d segments, %.3f bytes per operation, %d escapes" % (len(ops), len(recs), len(seg), ns, len(seg) / len(ops), n_esc)
    assert line in run(["info", coded]).stderr and "coded" not in run(["info", raw]).stderr
    # a sanity condition, no performance claim: 32 raw bits an operation against at most 10 model bits and the table
    v1, v2 = len(AR.read_archive(raw)["hipcigars"].parts[0][1]), len(AR.read_archive(coded)["hipcigars"].parts[0][1])
    assert v2 < v1
    print("hipcigars: version 1 %d bytes, version 2 %d bytes; %d operations, %.3f coded bytes per operation, %d escapes" % (v1, v2, len(ops), len(seg) / len(ops), n_esc))


def test_every_other_stream_is_byte_for_byte_the_same_and_version_1_is_as_before(tmp_path, inputs, archives):
    fa, fq = inputs
    raw, coded = archives
    assert streams(coded, skip=("info", "hipcigars")) == streams(raw, skip=("info", "hipcigars"))      # `hipmappings` included
    assert set(AR.read_archive(coded)) == set(AR.read_archive(raw))
    recs, rec_ops, ops = stored(raw)                                                       # (asserts version 1, four bytes an operation)
    assert AR.read_archive(raw)["hipcigars"].parts[0][1] == CR.pack_hipcigars(rec_ops, ops)
    out = str(tmp_path / "o.fastq")
    run(["decompress", "-G", fa, coded, out])
    assert open(out, "rb").read() == open(fq, "rb").read()
    run(["check", "-G", fa, coded])
    arc = str(tmp_path / "r.colord")
    r = run(["compress-ont", "-G", fa, "--mappings", "--cigars-coded", fq, arc], ok=False)
    assert r.returncode == 1 and "--cigars-coded needs --cigars" in r.stderr and not os.path.exists(arc)


def library_run(ctx, truth, cuts, packs, announce, coded):
    """tests/test_gpu_cli_cigars.py's library_run with the coded flag: -> (the records, the counts, the operations cl_ctx_cigars gives, what cigars_coded gives)"""
    import torch
    from util import golden
    from test_gpu_stream import params_of
    genome, seqs = truth
    prm = dict(params_of(golden("s6m_ont")), ci=2, f=4, sparse=0, frac_min=0.02)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)

    def arena_of(parts):
        return ctx.pack_reads(torch.from_numpy(np.concatenate(parts)), torch.from_numpy(np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)))
    chunks = [arena_of(seqs[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    gen = arena_of(genome)
    cmp_ = ctx.compressor(prm, None, None, None, expected_bases=int(off[-1]))
    ctx.set_mappings(True); ctx.set_cigars(True); ctx.set_cigars_coded(coded)
    try:
        cmp_.genome_add(gen)
        for c in chunks:
            cmp_.count_add(c)
        cmp_.count_finish()
        read_len, overlap = 20 * cmp_.info()["mean_read_len"], (prm["k"] - 1) * 10
        pseudo = arena_of([genome[s][a:a + ln] for s, a, ln in MR.pieces(SEQ_LEN, read_len, overlap)])
        cmp_.pseudo_reads(pseudo)
        cmp_.genome_geometry(SEQ_LEN, read_len, overlap)
        for c in chunks:
            cmp_.refs_add(c)
        cmp_.refs_finish()
        if announce:
            for c in chunks:
                cmp_.prepare(c, [0, c.n_reads])
        for c, a, b in zip(chunks, cuts[:-1], cuts[1:]):
            cmp_.encode(c, [0, c.n_reads], [p - a for p in packs if a <= p <= b])
        recs = cmp_.mappings()
        rec_ops, ops = cmp_.cigars()
        packed = cmp_.cigars_coded() if coded else None
    finally:
        ctx.set_cigars(False); ctx.set_mappings(False)
    cmp_.free(); pseudo.free(); gen.free()
    for c in chunks:
        c.free()
    return recs, rec_ops, ops, packed


def test_four_chunks_on_the_encode_lanes_decode_to_the_operations_of_one_chunk(ctx, truth):
    """the segment bytes depend on how the input was batched, the decoded operations do not"""
    cuts = [0, 13, 30, 46, 60]
    recs4, rec4, ops4, (crec4, seg4, no4, ns4) = library_run(ctx, truth, cuts, cuts, True, True)
    recs1, rec1, ops1, (crec1, seg1, no1, ns1) = library_run(ctx, truth, [0, 60], cuts, False, True)
    recs0, rec0, ops0, _ = library_run(ctx, truth, [0, 60], cuts, False, False)          # the raw operations of --cigars alone
    assert len(recs0) > 30 and np.array_equal(recs4, recs0) and np.array_equal(recs1, recs0)
    for rec, ops, crec, seg, no, ns in ((rec4, ops4, crec4, seg4, no4, ns4), (rec1, ops1, crec1, seg1, no1, ns1)):
        assert np.array_equal(rec, rec0) and np.array_equal(ops, ops0) and np.array_equal(crec, rec0)
        assert no == len(ops0) and np.array_equal(D.cigars_unpack_host(seg), ops0)
        assert every_segment_is_the_host_twins(seg, ops0) == ns
    assert ns4 > ns1 >= 1 and CR.invariants(recs0, rec0, ops0) == []                        # more batches, more segments: other bytes, the same operations
    assert not ctx.lib.cl_ctx_set_cigars_coded(ctx.h, 0)


def test_the_flag_is_refused_without_the_cigars(ctx):
    from colord_amd import _native as N
    ctx.set_mappings(True); ctx.set_cigars(False)
    try:
        with pytest.raises(N.ColordHipError) as x:
            ctx.set_cigars_coded(True)
        assert x.value.status == N.CL_E_INVALID and "cl_ctx_set_cigars" in str(x.value)
    finally:
        ctx.set_mappings(False)
