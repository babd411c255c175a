"""GPU suite of `colord_hip compress-* -G genome.fa --mappings --cigars`: the archive stores a `hipcigars` stream made on the device from
the tuple streams, one CIGAR per record of `hipmappings`; `info --mappings --cigar` prints the PAF with cg:Z:, `info --mappings --sam` SAM.  The input
is that of tests/test_gpu_cli_mappings.py (its generator is copied here): 60 reads of 2 - 5 kb on a three-sequence genome.  The truth test walks every
printed CIGAR over the genome and the read, base by base, with no tolerance."""
import hashlib
import os
import subprocess
import numpy as np
import pytest
from colord_amd import archive as AR
from colord_amd.fastq import ReadSet, write_fastq
import cigars_ref as CR
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
    substitution, insertion per base) -> (genome sequences, read sequences).  Every sequence gets reads, in shuffled order, and the strands
    alternate within a sequence, so that both strands of every sequence are met."""
    rng = np.random.default_rng(seed)
    genome = [rng.integers(0, 4, ln, dtype=np.uint8) for ln in SEQ_LEN]
    e_del, e_sub, e_ins = err
    plan = [(s, bool(i % 2)) for s, n in enumerate(per_seq) for i in range(n)]
    plan = [plan[i] for i in rng.permutation(len(plan))]
    seqs = []
    for sq, rev in plan:
        ln = int(rng.integers(2000, 5001))
        st = int(rng.integers(0, SEQ_LEN[sq] - ln))
        s = genome[sq][st:st + ln].copy()
        if rev:
            s = (3 - s[::-1]).astype(np.uint8)
        r = rng.random(ln)
        sub = (r >= e_del) & (r < e_del + e_sub)
        s[sub] = (s[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
        s = s[r >= e_del]
        ins = np.nonzero(rng.random(len(s)) < e_ins)[0]
        s = np.insert(s, ins, rng.integers(0, 4, len(ins)).astype(np.uint8))
        seqs.append(s.astype(np.uint8))
    return genome, seqs


@pytest.fixture(scope="module")
def truth():
    return reads_with_coordinates()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, truth):
    genome, seqs = truth
    d = tmp_path_factory.mktemp("cg_in")
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
    d = tmp_path_factory.mktemp("cg_arc")
    plain, mapped, both = str(d / "plain.colord"), str(d / "map.colord"), str(d / "cigars.colord")
    run(["compress-ont", "-G", fa] + SENSITIVE + [fq, plain])
    run(["compress-ont", "-G", fa, "--mappings"] + SENSITIVE + [fq, mapped])
    run(["compress-ont", "-G", fa, "--mappings", "--cigars"] + SENSITIVE + [fq, both])
    return plain, mapped, both


def stored(arc):
    a = AR.read_archive(arc)
    assert len(a["hipmappings"].parts) == 1 and len(a["hipcigars"].parts) == 1
    _, _, _, _, recs = MR.parse(a["hipmappings"].parts[0][1])
    b = a["hipcigars"].parts[0][1]
    version, op_bytes, nr, no = np.frombuffer(b[:8], "<u4").tolist() + np.frombuffer(b[8:24], "<u8").tolist()
    assert (version, op_bytes) == (1, 4) and len(b) == 24 + 4 * (nr + no)
    w = np.frombuffer(b[24:], "<u4")
    return recs, w[:nr].copy(), w[nr:].copy()


def streams(path, skip=("info",)):
    return {n: [(m, hashlib.sha256(p).hexdigest()) for m, p in s.parts] for n, s in AR.read_archive(path).items() if n not in skip}


def test_every_cigar_walks_its_read_over_the_genome(truth, archives):
    """Truth, exact: the printed cg:Z: walked over genome[ts:te] and over the read's [qs, qe) (reverse-complemented for `-`): every = column has equal
    bases, every X column differing ones, and the lengths consume both intervals exactly."""
    genome, seqs = truth
    recs, rec_ops, ops = stored(archives[2])
    assert len(recs) == len(rec_ops) > 30 and CR.invariants(recs, rec_ops, ops) == []
    lines = run(["info", "--mappings", "--cigar", archives[2]]).stdout.splitlines()
    assert lines == CR.paf_lines(recs, rec_ops, ops, SEQ_LEN, SEQ_NAMES) and len(lines) == len(recs)
    assert [line.rsplit("\t", 1)[0] for line in lines] == run(["info", "--mappings", archives[2]]).stdout.splitlines()      # the PAF of today and one column
    bad, seen, strands = [], set(), set()
    for line in lines:
        c = line.split("\t")
        q, qs, qe, strand, t, ts, te = int(c[0]), int(c[2]), int(c[3]), c[4], SEQ_NAMES.index(c[5]), int(c[7]), int(c[8])
        assert c[15].startswith("cg:Z:")
        read = seqs[q][qs:qe]
        if strand == "-":
            read = (3 - read[::-1]).astype(np.uint8)
        ref = genome[t][ts:te]
        i = j = 0
        for ch, n in CR.parse_text(c[15][5:]):
            seen.add(ch)
            if ch in "=X":
                same = read[i:i + n] == ref[j:j + n]
                if len(same) != n or (ch == "=" and not same.all()) or (ch == "X" and same.any()):
                    bad.append((line[:80], ch, n, i, j))
                    break
                i, j = i + n, j + n
            elif ch == "I":
                i += n
            else:
                j += n
        else:
            if (i, j) != (len(read), len(ref)):
                bad.append((line[:80], "lengths", i, len(read), j, len(ref)))
        strands.add(strand)
    assert not bad, bad[:5]
    assert seen == set("=XID") and strands == {"+", "-"}                                   # not vacuous: every operation, both strands
    print("records %d, operations %d, %.1f per record; hipcigars %d bytes" % (len(recs), len(ops), len(ops) / len(recs), 24 + 4 * (len(recs) + len(ops))))


def test_sam_parses_and_agrees_with_the_paf(archives):
    recs, rec_ops, ops = stored(archives[2])
    out = run(["info", "--mappings", "--sam", archives[2]]).stdout.splitlines()
    assert out == CR.sam_lines(recs, rec_ops, ops, SEQ_LEN, SEQ_NAMES)
    head, body = [x for x in out if x.startswith("@")], [x.split("\t") for x in out if not x.startswith("@")]
    assert head == ["@HD\tVN:1.6\tSO:unknown"] + ["@SQ\tSN:%s\tLN:%d" % (n, ln) for n, ln in zip(SEQ_NAMES, SEQ_LEN)]
    paf = [x.split("\t") for x in run(["info", "--mappings", "--cigar", archives[2]]).stdout.splitlines()]
    assert len(body) == len(paf) == len(recs)
    first = set()
    for s, p in zip(body, paf):
        assert len(s) == 12 and s[0] == p[0] and s[2] == p[5] and int(s[3]) == int(p[7]) + 1 and s[4] == "255" and s[6:11] == ["*", "0", "0", "*", "*"]
        flag = int(s[1])
        assert flag & ~(16 | 2048) == 0 and bool(flag & 16) == (p[4] == "-") and bool(flag & 2048) == (s[0] in first)
        first.add(s[0])
        cg = CR.parse_text(s[5])
        inner = [x for x in cg if x[0] != "H"]
        assert "".join("%d%s" % (n, c) for c, n in inner) == p[15][5:] and all(c != "H" for c, _ in cg[1:-1])
        assert sum(n for c, n in cg if c in "=XIH") == int(p[1])                           # the query length with its hard clips is qlen
        assert int(s[11][5:]) == sum(n for c, n in inner if c in "XID") and s[11].startswith("NM:i:")
        lead = cg[0][1] if cg[0][0] == "H" else 0                                         # the clips are swapped for `-`
        assert lead == (int(p[1]) - int(p[3]) if p[4] == "-" else int(p[2]))
    named = run(["info", "--mappings", "--sam", "--names", archives[2]]).stdout.splitlines()
    assert [x.split("\t")[0] for x in named if not x.startswith("@")] == ["read_%s" % s[0] for s in body]
    assert "cigars: %d operations of %d mapping records" % (len(ops), len(recs)) in run(["info", archives[2]]).stderr and "cigars" not in run(["info", archives[1]]).stderr


def test_without_the_flag_every_byte_is_as_before_and_the_decoders_ignore_the_stream(tmp_path, inputs, archives):
    fa, fq = inputs
    plain, mapped, both = archives
    assert "hipcigars" not in AR.read_archive(mapped) and "hipcigars" not in AR.read_archive(plain)
    assert streams(mapped, skip=("info", "hipmappings")) == streams(plain)                # --mappings alone: the archive of the parent's options
    assert streams(both, skip=("info", "hipcigars")) == streams(mapped)                   # `hipmappings` included, byte for byte
    assert set(AR.read_archive(both)) == set(AR.read_archive(plain)) | {"hipmappings", "hipcigars"}
    out = str(tmp_path / "o.fastq")
    run(["decompress", "-G", fa, both, out])
    assert open(out, "rb").read() == open(fq, "rb").read()
    run(["check", "-G", fa, both])
    r = run(["info", "--mappings", "--cigar", mapped], ok=False)
    assert r.returncode == 1 and "no CIGARs are stored" in r.stderr


def test_reference_decompressor_ignores_the_stream(tmp_path, inputs, archives):
    fa, fq = inputs
    ref = os.path.join(ROOT, "oracle", "_ref", "colord")
    assert os.path.exists(ref), "oracle/_ref/colord is built by build()"
    for a, out in ((archives[0], "p.fastq"), (archives[2], "c.fastq")):
        subprocess.check_call([ref, "decompress", "-G", fa, a, str(tmp_path / out)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert open(str(tmp_path / "p.fastq"), "rb").read() == open(str(tmp_path / "c.fastq"), "rb").read() == open(fq, "rb").read()


def library_run(ctx, truth, cuts, packs, announce):
    """the 60 reads through the chunked compressor of the library (cl_compressor_*) with the genome's pieces as pseudo reads, cut into chunks at `cuts`
    and into reader packs at `packs` (the encoder's adaptive decisions are per pack) -> (the lifted records, the counts, the operations)"""
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
    ctx.set_mappings(True); ctx.set_cigars(True)
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
    finally:
        ctx.set_cigars(False); ctx.set_mappings(False)
    ctx.set_mappings(True); ctx.set_cigars(True); ctx.set_cigars(False); ctx.set_mappings(False)      # (nothing is left on the shared context)
    assert ctx.cigars()[0].size == 0
    cmp_.free(); pseudo.free(); gen.free()
    for c in chunks:
        c.free()
    return recs, rec_ops, ops


def test_the_same_cigars_from_four_chunks_on_the_encode_lanes(ctx, truth):
    """cut in four chunks of one pack each and announced ahead, stage A runs on the encode lanes, which finish out of order: the batches are merged by
    their first read, the CIGARs as the records.  One chunk of the same four packs on the caller's context must give the same counts and operations."""
    cuts = [0, 13, 30, 46, 60]
    on_lanes = library_run(ctx, truth, cuts, cuts, announce=True)
    one_chunk = library_run(ctx, truth, [0, 60], cuts, announce=False)
    assert len(on_lanes[0]) > 30 and all(np.array_equal(a, b) for a, b in zip(on_lanes, one_chunk))
    assert CR.invariants(*on_lanes) == []


def test_the_flag_is_refused_without_the_mappings(ctx, tmp_path, inputs):
    from colord_amd import _native as N
    ctx.set_mappings(False)
    with pytest.raises(N.ColordHipError) as x:
        ctx.set_cigars(True)
    assert x.value.status == N.CL_E_INVALID and "cl_ctx_set_mappings" in str(x.value)
    arc = str(tmp_path / "r.colord")
    r = run(["compress-ont", "-G", inputs[0], "--cigars", inputs[1], arc], ok=False)
    assert r.returncode == 1 and "--cigars needs --mappings" in r.stderr and not os.path.exists(arc)
