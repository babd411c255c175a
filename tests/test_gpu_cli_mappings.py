"""GPU suite of `colord_hip compress-* -G genome.fa --mappings`: the archive stores a `hipmappings` stream made on the device from the
tuple streams and lifted to the genome's sequences; `info --mappings` prints it as PAF with the FASTA's names, as a coverage track, as a summary.
The input is about 60 reads of 2 - 5 kb whose place on a three-sequence genome (150 kb, 40 kb, 10 kb) is known base by base: the truth test asks
of every record with anchor bases the right sequence, an interval that meets the read's true one, and the right strand."""
import hashlib
import json
import os
import subprocess
import numpy as np
import pytest
from colord_amd import archive as AR
from colord_amd.fastq import ReadSet, write_fastq
import overlaps_ref as OR
import mappings_ref as MR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
SEQ_LEN = [150_000, 40_000, 10_000]
SEQ_NAMES = ["chrA", "chrB", "chrC"]
# k-mers seen twice are kept (once on the genome, once in a read), one in four of them sampled, a candidate from 2 % of shared m-mers on: at a
# coverage of one a read's only neighbour is the genome
SENSITIVE = ["-L", "2", "-f", "4", "--min-mmer-frac", "0.02"]


def run(args, ok=True):
    r = subprocess.run([CLI] + args, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r


def reads_with_coordinates(seed=20, per_seq=(45, 10, 5), err=(0.02, 0.03, 0.02)):
    """60 reads of 2 - 5 kb from either strand of a random three-sequence genome with the ONT error rates of colord_amd/synth.py (deletion,
    substitution, insertion per base) -> (genome sequences, read sequences, per read its sequence, the coordinate of every base, strands); an
    inserted base takes its left neighbour's coordinate (the first base's when it is the first).  Every sequence gets reads, in shuffled order,
    and the strands alternate within a sequence, so that both strands of every sequence are met."""
    rng = np.random.default_rng(seed)
    genome = [rng.integers(0, 4, ln, dtype=np.uint8) for ln in SEQ_LEN]
    e_del, e_sub, e_ins = err
    plan = [(s, bool(i % 2)) for s, n in enumerate(per_seq) for i in range(n)]
    plan = [plan[i] for i in rng.permutation(len(plan))]
    seqs, where, coords, strands = [], [], [], []
    for sq, rev in plan:
        ln = int(rng.integers(2000, 5001))
        st = int(rng.integers(0, SEQ_LEN[sq] - ln))
        s, c = genome[sq][st:st + ln].copy(), np.arange(st, st + ln)
        if rev:
            s, c = (3 - s[::-1]).astype(np.uint8), c[::-1].copy()
        r = rng.random(ln)
        sub = (r >= e_del) & (r < e_del + e_sub)
        s[sub] = (s[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
        s, c = s[r >= e_del], c[r >= e_del]
        ins = np.nonzero(rng.random(len(s)) < e_ins)[0]
        s = np.insert(s, ins, rng.integers(0, 4, len(ins)).astype(np.uint8))
        c = np.insert(c, ins, c[np.maximum(ins - 1, 0)])
        seqs.append(s.astype(np.uint8)); where.append(sq); coords.append(c); strands.append(rev)
    return genome, seqs, where, coords, strands


@pytest.fixture(scope="module")
def truth():
    return reads_with_coordinates()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, truth):
    genome, seqs, _, _, _ = truth
    d = tmp_path_factory.mktemp("map_in")
    fa, fq = str(d / "genome.fa"), str(d / "reads.fastq")
    lut = np.frombuffer(b"ACGT", np.uint8)
    with open(fa, "wb") as f:
        for name, g in zip(SEQ_NAMES, genome):
            f.write(b">" + name.encode() + b" a random sequence\n")
            text = lut[g].tobytes()
            f.write(b"\n".join(text[i:i + 60] for i in range(0, len(text), 60)) + b"\n")
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    quals = np.frombuffer(b"%+5C", np.uint8)[np.random.default_rng(1).choice(4, int(off[-1]))]
    write_fastq(fq, ReadSet(np.concatenate(seqs), off, quals, [b"read_%d len=%d" % (i, len(s)) for i, s in enumerate(seqs)], [False] * len(seqs), True))
    return fa, fq


@pytest.fixture(scope="module")
def archives(tmp_path_factory, inputs):
    fa, fq = inputs
    d = tmp_path_factory.mktemp("map_arc")
    plain, again, mapped = str(d / "plain.colord"), str(d / "again.colord"), str(d / "map.colord")
    run(["compress-ont", "-G", fa] + SENSITIVE + [fq, plain])
    run(["compress-ont", "-G", fa] + SENSITIVE + [fq, again])
    run(["compress-ont", "-G", fa, "--mappings", "--edit-profile"] + SENSITIVE + [fq, mapped])
    return plain, again, mapped


def stored(arc):
    a = AR.read_archive(arc)
    assert "hipmappings" in a and len(a["hipmappings"].parts) == 1
    return MR.parse(a["hipmappings"].parts[0][1])


def streams(path, skip=("info", "hipmappings", "hipedits")):
    return {n: [(m, hashlib.sha256(p).hexdigest()) for m, p in s.parts] for n, s in AR.read_archive(path).items() if n not in skip}


def test_records_lie_where_the_reads_come_from(truth, inputs, archives):
    """No tolerance: an anchor is an exact match of anchor-length bases, and a random 200-kb genome repeats none often enough to place a read
    elsewhere.  The counts printed here are the ones DESIGN.md 4m quotes."""
    _, seqs, where, coords, strands = truth
    seq_len, names, read_len, overlap, recs = stored(archives[2])
    mean = sum(len(s) for s in seqs) / len(seqs)
    assert (seq_len, names) == (SEQ_LEN, SEQ_NAMES) and 0.98 * 20 * mean <= read_len <= 1.02 * 20 * mean
    # (pseudo reads of 20 x the mean read length as the compressor estimates it, from the 1-in-4 sample of the k-mers: about 54 000 samples,
    # a relative deviation of 0.4 %; the piece counts below are what the rest of the test needs)
    assert [len([p for p in MR.pieces(SEQ_LEN, read_len, overlap) if p[0] == s]) for s in range(3)] == [3, 1, 1]
    f = {k: recs[:, i].astype(np.int64) for i, k in enumerate(MR.FIELDS)}
    prof = json.loads(run(["info", "--edit-profile", "--json", archives[2]]).stdout)
    step = read_len - overlap
    print("reads %d, by script %d, reads mapped %d, records %d, with anchors %d" % (len(seqs), int(prof["kind_reads"][2]), len(set(f["q"].tolist())), len(recs), int((f["anchor_bases"] > 0).sum())))
    assert (f["flags"] & MR.GENOME).all() and (f["flags"] < 8).all() and (f["qs"] < f["qe"]).all() and (f["ts"] < f["te"]).all() and (f["te"] <= f["tlen"]).all()
    assert (f["qlen"] == np.array([len(seqs[q]) for q in f["q"]])).all() and (f["tlen"] == np.array(SEQ_LEN)[f["t"]]).all() and (np.diff(f["q"]) >= 0).all()
    bad, met, pieces_of_first = [], set(), set()
    for i in np.nonzero(f["anchor_bases"] > 0)[0]:
        q, t = int(f["q"][i]), int(f["t"][i])
        cq = coords[q][f["qs"][i]:f["qe"][i]]
        meet = max(cq.min(), f["ts"][i]) <= min(cq.max(), f["te"][i] - 1)
        rev = bool(f["flags"][i] & OR.REV)
        if t != where[q] or not meet or rev != strands[q]:
            bad.append((recs[i].tolist(), where[q], int(cq.min()), int(cq.max()), strands[q]))
        met.add((t, rev))
        if t == 0:                                                                       # the pieces of the first sequence the record may lie on
            pieces_of_first.add(tuple(p for p in range(-(-SEQ_LEN[0] // step)) if p * step <= f["ts"][i] and f["te"][i] <= p * step + read_len))
    assert not bad, bad[:5]
    # not vacuous: records on every sequence, on both strands of each, and on at least two pieces of the first
    assert met == {(t, r) for t in range(3) for r in (False, True)}
    assert all(pieces_of_first) and len({p for ps in pieces_of_first if len(ps) == 1 for p in ps}) >= 2


def test_info_prints_paf_with_the_sequence_names_and_a_coverage_that_adds_up(archives):
    seq_len, names, _, _, recs = stored(archives[2])
    lines = run(["info", "--mappings", archives[2]]).stdout.splitlines()
    assert lines == MR.paf_lines(recs, seq_len, names) and len(lines) == len(recs) > 0
    for line in lines:
        c = line.split("\t")
        assert len(c[:12]) == 12 and len(c) == 15 and c[5] in SEQ_NAMES and int(c[6]) == SEQ_LEN[SEQ_NAMES.index(c[5])] and c[4] in "+-" and c[11] == "255"
        assert 0 <= int(c[2]) < int(c[3]) <= int(c[1]) and 0 <= int(c[7]) < int(c[8]) <= int(c[6]) and int(c[9]) <= int(c[10])
    ids = ["read_%d" % i for i in range(60)]
    assert run(["info", "--mappings", "--names", archives[2]]).stdout.splitlines() == MR.paf_lines(recs, seq_len, names, read_names=ids)
    total = int((recs[:, 7].astype(np.int64) - recs[:, 6]).sum())
    for w in (1000, 7777):
        got = run(["info", "--mappings", "--coverage", str(w), archives[2]]).stdout.splitlines()
        assert got == MR.coverage_lines(recs, seq_len, names, w)
        rows = [x.split("\t") for x in got]
        assert sum(round(float(x[3]) * (int(x[2]) - int(x[1]))) for x in rows) == total and len(rows) == sum(-(-ln // w) for ln in SEQ_LEN)
    s = json.loads(run(["info", "--mappings", "--summary", "--json", archives[2]]).stdout)
    assert s == MR.summary(recs, 60)
    assert "mappings: %d records" % len(recs) in run(["info", archives[2]]).stderr and "mappings" not in run(["info", archives[0]]).stderr


def test_without_the_flag_every_byte_is_as_before_and_the_decoders_ignore_the_stream(tmp_path, inputs, archives):
    fa, fq = inputs
    plain, again, mapped = archives
    assert streams(plain, skip=("info",)) == streams(again, skip=("info",)) and "hipmappings" not in AR.read_archive(plain)
    assert streams(mapped) == streams(plain)                                             # every stream but `info` and the two views
    assert set(AR.read_archive(mapped)) == set(AR.read_archive(plain)) | {"hipmappings", "hipedits"}
    for arc in (plain, mapped):
        out = str(tmp_path / "o.fastq")
        run(["decompress", "-G", fa, arc, out])
        assert open(out, "rb").read() == open(fq, "rb").read()
    run(["check", "-G", fa, mapped])


def library_run(ctx, truth, cuts, announce):
    """the 60 reads through the chunked compressor of the library (cl_compressor_*) with the genome's pieces as pseudo reads, every chunk one pack:
    -> (the lifted records, the dna parts)"""
    import torch
    from util import golden
    from test_gpu_stream import params_of
    genome, seqs, _, _, _ = truth
    prm = dict(params_of(golden("s6m_ont")), ci=2, f=4, sparse=0, frac_min=0.02)
    lens = np.array([len(s) for s in seqs])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    bases = np.concatenate(seqs)

    def arena_of(parts):
        return ctx.pack_reads(torch.from_numpy(np.concatenate(parts)), torch.from_numpy(np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)))
    chunks = [arena_of(seqs[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    gen = arena_of(genome)
    cmp_ = ctx.compressor(prm, None, None, None, expected_bases=int(off[-1]))
    ctx.set_mappings(True)
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
        dna = []
        for c in chunks:
            d, ds, _, _, _ = cmp_.encode(c, [0, c.n_reads], [0, c.n_reads])
            dna.append((d.cpu().numpy().tobytes(), [int(x) for x in ds]))
        recs = cmp_.mappings()
    finally:
        ctx.set_mappings(False)
    ctx.set_mappings(True); ctx.set_mappings(False)                             # (nothing is left on the shared context)
    cmp_.free(); pseudo.free(); gen.free()
    for c in chunks:
        c.free()
    return recs, dna, (read_len, overlap)


def test_the_same_records_from_several_chunks_on_the_encode_lanes(ctx, truth):
    """The command line cuts chunks at packs of 4 Mi symbols, so the 60 reads are one chunk there; here they go through the library's chunked
    compressor, cut in four chunks of one pack each and announced ahead, so that stage A runs on both encode lanes, which finish out of order: the
    batches are merged by their first read.  The same four packs coded call by call on the caller's context must give the same records and parts."""
    _, seqs, where, _, strands = truth
    cuts = [0, 13, 30, 46, 60]
    on_lanes, dna_lanes, geo = library_run(ctx, truth, cuts, announce=True)
    in_turn, dna_turn, _ = library_run(ctx, truth, cuts, announce=False)
    assert len(on_lanes) > 0 and np.array_equal(on_lanes, in_turn) and dna_lanes == dna_turn
    f = {k: on_lanes[:, i].astype(np.int64) for i, k in enumerate(MR.FIELDS)}
    assert (np.diff(f["q"]) >= 0).all() and all(len(set(f["q"][(f["q"] >= a) & (f["q"] < b)].tolist())) > 0 for a, b in zip(cuts[:-1], cuts[1:]))      # every chunk left records, in input order
    assert (f["flags"] & MR.GENOME).all() and (f["te"] <= f["tlen"]).all() and (f["tlen"] == np.array(SEQ_LEN)[f["t"]]).all()
    anchored = f["anchor_bases"] > 0
    assert (f["t"][anchored] == np.array(where)[f["q"][anchored]]).all() and ((f["flags"][anchored] & OR.REV > 0) == np.array(strands)[f["q"][anchored]]).all()


@pytest.mark.parametrize("extra,text", [(["--gpus", "2", "--gpu-list", "0,0", "--transport", "host"], "--mappings is not available with --gpus > 1"),
                                        (["--domains", "2"], "--mappings is not available with --domains > 1"), (["--overlaps"], "--mappings is not available with --overlaps")],
                         ids=["gpus", "domains", "overlaps"])
def test_refused_combinations(tmp_path, inputs, extra, text):
    fa, fq = inputs
    arc = str(tmp_path / "r.colord")
    r = run(["compress-ont", "-G", fa, "--mappings"] + extra + [fq, arc], ok=False)
    assert r.returncode == 1 and text in r.stderr and not os.path.exists(arc)


def test_the_flag_without_a_genome_is_refused(tmp_path, inputs):
    arc = str(tmp_path / "r.colord")
    r = run(["compress-ont", "--mappings", inputs[1], arc], ok=False)
    assert r.returncode == 1 and "--mappings needs a reference genome (-G)" in r.stderr and not os.path.exists(arc)
