"""GPU suite of `colord_hip compress-* -G genome.fa --pileup`, the truth test: a random genome of three sequences (30 kb, 12 kb, 5 kb), a
MUTATED copy of it with 20 planted single-base variants, and 400 reads of 2 - 5 kb from either strand of the mutated copy with ONT error rates.  The
reads are compressed against the ORIGINAL genome with --pileup --mappings: the sites of the `hippileup` stream must hold the planted variants."""
import os
import subprocess
import numpy as np
import pytest
from colord_amd import archive as AR
from colord_amd.fastq import ReadSet, write_fastq
import mappings_ref as MR
import pileup_ref as PR
from test_gpu_cli_mappings import SENSITIVE, run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ_LEN = [30_000, 12_000, 5_000]
SEQ_NAMES = ["chrA", "chrB", "chrC"]
N_READS, N_SNV, APART = 400, 20, 300
ERR = (0.02, 0.03, 0.02)                                       # deletion, substitution, insertion per base, as tests/test_gpu_cli_mappings.py


def planted(seed=41):
    """-> (original sequences, mutated sequences, [(sequence, position, original base, planted base)]): the variants lie at least APART bases from
    each other and from any sequence end"""
    rng = np.random.default_rng(seed)
    genome = [rng.integers(0, 4, ln, dtype=np.uint8) for ln in SEQ_LEN]
    base = np.concatenate([[0], np.cumsum(SEQ_LEN)])
    taken = []
    while len(taken) < N_SNV:
        x = int(rng.integers(0, base[-1]))
        s = int(np.searchsorted(base, x, side="right")) - 1
        p = x - int(base[s])
        if APART <= p < SEQ_LEN[s] - APART and all(t[0] != s or abs(t[1] - p) >= APART for t in taken):
            taken.append((s, p))
    mutated = [g.copy() for g in genome]
    snv = []
    for s, p in sorted(taken):
        alt = (int(genome[s][p]) + int(rng.integers(1, 4))) % 4
        mutated[s][p] = alt
        snv.append((s, p, int(genome[s][p]), alt))
    return genome, mutated, snv


def reads_of(mutated, n_reads=N_READS, seed=42):
    """reads of 2 - 5 kb from either strand of the mutated copy, spread over the sequences by their lengths -> (sequences, per read its sequence, the
    true coordinate of every base, strands); an inserted base takes its left neighbour's coordinate"""
    rng = np.random.default_rng(seed)
    e_del, e_sub, e_ins = ERR
    where = rng.choice(3, n_reads, p=np.array(SEQ_LEN) / sum(SEQ_LEN))
    seqs, coords, strands = [], [], []
    for i, sq in enumerate(where):
        ln = int(rng.integers(2000, min(5000, SEQ_LEN[sq] - 1) + 1))
        st = int(rng.integers(0, SEQ_LEN[sq] - ln))
        s, c = mutated[sq][st:st + ln].copy(), np.arange(st, st + ln)
        rev = bool(i % 2)
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
    return seqs, [int(w) for w in where], coords, strands


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    genome, mutated, snv = planted()
    seqs, where, coords, strands = reads_of(mutated)
    d = tmp_path_factory.mktemp("pile_in")
    fa, fq, arc = str(d / "original.fa"), str(d / "reads.fastq"), str(d / "pile.colord")
    lut = np.frombuffer(b"ACGT", np.uint8)
    with open(fa, "wb") as f:
        for name, g in zip(SEQ_NAMES, genome):
            f.write(b">" + name.encode() + b" a random sequence\n")
            text = lut[g].tobytes()
            f.write(b"\n".join(text[i:i + 60] for i in range(0, len(text), 60)) + b"\n")
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    quals = np.frombuffer(b"%+5C", np.uint8)[np.random.default_rng(1).choice(4, int(off[-1]))]
    write_fastq(fq, ReadSet(np.concatenate(seqs), off, quals, [b"read_%d len=%d" % (i, len(s)) for i, s in enumerate(seqs)], [False] * len(seqs), True))
    run(["compress-ont", "-G", fa, "--pileup", "--mappings"] + SENSITIVE + [fq, arc])
    return dict(genome=genome, snv=snv, fa=fa, fq=fq, arc=arc, n_reads=len(seqs))


def test_the_planted_variants_are_sites(made, tmp_path):
    """Exact: the stream's `match` and `sub` totals are the sums of `matches` and `subst` over the `hipmappings` records — two independent walks of
    the same scripts —, every site's `ref` is the original genome's base, `decompress` gives the input back, and the reference's decompressor (where
    it is built) reads the archive.  Planted variants: one counts as covered when at least 10 mapping records contain its position; every covered
    one must be a site of the planted base's kind, at most 1 in 10 of the covered ones may be missed (a cap: misplaced gaps next to a variant can
    move a column), and at least half of the 20 must be covered, or the test is empty.  The counts printed here are the ones DESIGN.md 4n quotes."""
    a = AR.read_archive(made["arc"])
    assert "hippileup" in a and len(a["hippileup"].parts) == 1 and "hipmappings" in a
    S = PR.parse(a["hippileup"].parts[0][1])
    seq_len, names, _, _, recs = MR.parse(a["hipmappings"].parts[0][1])
    assert (S["seq_len"], S["names"], S["thresholds"]) == (SEQ_LEN, SEQ_NAMES, PR.DEFAULTS) and (seq_len, names) == (SEQ_LEN, SEQ_NAMES)
    assert S["totals"]["match"] == int(recs[:, 8].astype(np.int64).sum()) and S["totals"]["sub"] == int(recs[:, 9].astype(np.int64).sum())
    assert 0 < len(set(recs[:, 0].tolist())) <= S["totals"]["reads"] <= made["n_reads"]        # (a read with a record has an aligned column on a piece)
    sites = S["sites"]
    assert all(int(r[2]) == int(made["genome"][r[0]][r[1]]) for r in sites)
    by_place = {(int(r[0]), int(r[1])): r for r in sites}
    covered, found, missed = 0, 0, []
    for s, p, ref, alt in made["snv"]:
        depth = int(((recs[:, 1] == s) & (recs[:, 6] <= p) & (p < recs[:, 7])).sum())
        if depth < 10:
            continue
        covered += 1
        r = by_place.get((s, p))
        if r is not None and int(r[3]) == alt and int(r[2]) == ref:
            found += 1
        else:
            missed.append((s, p, ref, alt, depth, None if r is None else r.tolist()))
    planted_places = {(s, p) for s, p, _, _ in made["snv"]}
    print("planted %d, covered %d, found %d, sites %d, sites that are not planted %d; reads on genome pieces %d of %d, covered positions %d, mean depth %.1f"
          % (N_SNV, covered, found, len(sites), sum(1 for k in by_place if k not in planted_places), S["totals"]["reads"], made["n_reads"], S["totals"]["covered"],
             (S["totals"]["match"] + S["totals"]["sub"] + S["totals"]["del"]) / max(1, S["totals"]["covered"])))
    assert 2 * covered >= N_SNV, "too few planted variants are covered: the test is empty"
    assert 10 * (covered - found) <= covered, missed
    out = str(tmp_path / "o.fastq")
    run(["decompress", "-G", made["fa"], made["arc"], out])
    assert open(out, "rb").read() == open(made["fq"], "rb").read()
    run(["check", "-G", made["fa"], made["arc"]])
    ref_bin = os.path.join(ROOT, "oracle", "_ref", "colord")
    if os.path.exists(ref_bin):                                                           # the reference's decompressor never sees the stream
        ref_out = str(tmp_path / "r.fastq")
        subprocess.check_call([ref_bin, "decompress", "-G", made["fa"], made["arc"], ref_out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        assert open(ref_out, "rb").read() == open(made["fq"], "rb").read()


def test_info_prints_what_the_stream_holds(made):
    a = AR.read_archive(made["arc"])
    S = PR.parse(a["hippileup"].parts[0][1])
    assert run(["info", "--pileup", made["arc"]]).stdout.splitlines() == PR.tsv_lines(S["sites"], SEQ_NAMES)
    assert run(["info", "--pileup", "--min-alt", "6", "--min-frac", "0.5", made["arc"]]).stdout.splitlines() == PR.tsv_lines(S["sites"], SEQ_NAMES, 6, 500)
    assert run(["info", "--pileup", "--vcf", made["arc"]]).stdout.splitlines() == PR.vcf_lines(S["sites"], SEQ_LEN, SEQ_NAMES)
    import json
    assert json.loads(run(["info", "--pileup", "--summary", "--json", made["arc"]]).stdout) == PR.summary(S)
    assert "pileup: %d sites on the 3 sequences" % len(S["sites"]) in run(["info", made["arc"]]).stderr


def library_run(ctx, genome, seqs, cuts, announce):
    """the reads through the chunked compressor of the library (cl_compressor_*) with the genome's pieces as pseudo reads, every chunk one pack, the
    context's pileup flag on -> (columns, totals, sites, the dna parts)"""
    import torch
    from util import golden
    from test_gpu_stream import params_of
    prm = dict(params_of(golden("s6m_ont")), ci=2, f=4, sparse=0, frac_min=0.02)
    total = sum(len(s) for s in seqs)

    def arena_of(parts):
        return ctx.pack_reads(torch.from_numpy(np.concatenate(parts)), torch.from_numpy(np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)))
    chunks = [arena_of(seqs[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    gen = arena_of(genome)
    cmp_ = ctx.compressor(prm, None, None, None, expected_bases=total)
    ctx.set_pileup(True)
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
        p = cmp_.pileup()
        out = (p.columns(), p.totals(), p.sites(), dna)
    finally:
        ctx.set_pileup(False)
    cmp_.free(); pseudo.free(); gen.free()
    for c in chunks:
        c.free()
    return out


def test_the_encode_lanes_add_into_one_table(ctx):
    """The command line cuts chunks at packs of 4 Mi symbols, so the 400 reads are one chunk there; here they go through the library's chunked
    compressor, cut in four chunks of one pack each and announced ahead, so that stage A — and with it the walk — runs on the encode lanes, which
    add into the compressor's ONE table at the same time.  The same four packs coded call by call on the caller's context must give the same
    table, totals, sites and parts: integer atomics, no order in the result."""
    genome, mutated, snv = planted()
    seqs, _, _, _ = reads_of(mutated)
    cuts = [0, 90, 210, 305, 400]
    cols_l, tot_l, sites_l, dna_l = library_run(ctx, genome, seqs, cuts, announce=True)
    cols_t, tot_t, sites_t, dna_t = library_run(ctx, genome, seqs, cuts, announce=False)
    assert np.array_equal(cols_l, cols_t) and tot_l == tot_t and np.array_equal(sites_l, sites_t) and dna_l == dna_t
    assert cols_l.shape == (sum(SEQ_LEN), 8) and np.array_equal(cols_l[:, 7], np.concatenate(genome)) and tot_l["reads"] > 300 and tot_l["covered"] > 40_000
    c = cols_l.astype(np.int64)
    assert tot_l["match"] == c[:, 0].sum() and tot_l["sub"] == c[:, 1:5].sum() and tot_l["del"] == c[:, 5].sum() and tot_l["ins"] == c[:, 6].sum()
    assert np.array_equal(sites_l, PR.sites_of(c, np.concatenate([[0], np.cumsum(SEQ_LEN)]), *PR.DEFAULTS))          # the sites are the table's
    found = {(int(r[0]), int(r[1])): int(r[3]) for r in sites_l}
    assert sum(1 for s, p, _, alt in snv if found.get((s, p)) == alt) >= N_SNV // 2


@pytest.mark.parametrize("extra,text", [(["--gpus", "2", "--gpu-list", "0,0", "--transport", "host"], "--pileup is not available with --gpus > 1"),
                                        (["--domains", "2"], "--pileup is not available with --domains > 1"), (["--overlaps"], "--pileup is not available with --overlaps")],
                         ids=["gpus", "domains", "overlaps"])
def test_refused_combinations(tmp_path, made, extra, text):
    arc = str(tmp_path / "r.colord")
    r = run(["compress-ont", "-G", made["fa"], "--pileup"] + extra + [made["fq"], arc], ok=False)
    assert r.returncode == 1 and text in r.stderr and not os.path.exists(arc)
