"""GPU suite of `colord_hip compress-* --kmer-spectrum`: the archive stores a `hipkmers` stream counted on the device from the
sorted k-mers of pass 1; `info --kmer-spectrum --json` prints it.  The judge is tests/kspec_ref.py over the k-mers the oracle scans from the
same reads (tests/data/M.bovis.fastq.gz, 100 reads, `compress-ont`: the parameters of c1_ont_default; with -G -s those of c4_ont_genome)."""
import gzip
import hashlib
import json
import os
import subprocess
import numpy as np
import pytest
from colord_amd import archive as AR
from oracle import pyoracle as O
from util import golden
import kspec_ref as K
from test_kspec_cpu import judged, printed as spectrum_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")


def run(args, ok=True):
    r = subprocess.run([CLI] + args, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ks_in") / "M.bovis.fastq")
    open(path, "wb").write(gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis.fastq.gz"), "rb").read())
    return path


def printed(arc, cfg="c1_ont_default", sets=1, flags=0):
    """the JSON of `info --kmer-spectrum --json` and its spectrum; the header states the parameters of cfg, the stored payload is the judge's packing"""
    a = AR.read_archive(arc)
    assert "hipkmers" in a and len(a["hipkmers"].parts) == 1 and a["hipkmers"].parts[0][0] == 0
    payload = a["hipkmers"].parts[0][1]
    o = json.loads(run(["info", "--kmer-spectrum", "--json", arc]).stdout)
    g = golden(cfg)
    assert [o[x] for x in ("version", "flags", "k", "f", "ci", "cs", "sets")] == [1, flags, g.p("k"), g.p("f"), g.p("ci"), g.p("cs"), sets]
    got = spectrum_of(o)
    assert K.pack_hipkmers(got, o["k"], o["f"], o["ci"], o["cs"], sets=sets, flags=flags) == payload and len(payload) == 32 + 8 * K.WORDS
    return o, got


def streams(path, skip=("info", "hipkmers")):
    return {n: [(m, hashlib.sha256(p).hexdigest()) for m, p in s.parts] for n, s in AR.read_archive(path).items() if n not in skip}


@pytest.fixture(scope="module")
def plain_archive(tmp_path_factory, fq):
    arc = str(tmp_path_factory.mktemp("ks_base") / "plain.colord")
    run(["compress-ont", fq, arc])
    return arc


def test_the_spectrum_is_stored_and_printed_and_no_other_byte_changes(tmp_path, fq, plain_archive):
    arc = str(tmp_path / "a.colord")
    run(["compress-ont", "--kmer-spectrum", fq, arc])
    want = judged("c1_ont_default")
    o, got = printed(arc)
    assert K.same(got, want) is None, K.same(got, want)
    g = golden("c1_ont_default")
    d = K.derived(want, o["f"], o["ci"], o["cs"])
    assert {k: o["derived"][k] for k in ("kept_distinct", "kept_kmers")} == {"kept_distinct": g.p("n_unique"), "kept_kmers": g.p("total_count_filtered")}
    assert o["derived"]["estimates"] is True and o["derived"]["peak"] is None and d["peak"] is None
    assert o["derived"]["below_ci_distinct"] == d["below_ci_distinct"] and o["derived"]["saturated_kmers"] == d["saturated_kmers"]
    assert streams(arc) == streams(plain_archive)                               # every stream but `info` and `hipkmers`
    assert "hipkmers" not in AR.read_archive(plain_archive) and set(AR.read_archive(arc)) == set(AR.read_archive(plain_archive)) | {"hipkmers"}
    i = run(["info", arc])
    assert "k-mer spectrum: %d sampled k-mers (1 in %d), %d distinct" % (want["kmers"], o["f"], want["distinct"]) in i.stderr
    t = run(["info", "--kmer-spectrum", arc]).stdout
    assert "1-in-f hash sample" in t and "distinct: %d\n" % want["distinct"] in t and "peak: none" in t
    out = str(tmp_path / "o.fastq")
    run(["decompress", arc, out])                                               # the decoders ignore the stream
    run(["decompress", plain_archive, str(tmp_path / "p.fastq")])
    assert open(out, "rb").read() == open(str(tmp_path / "p.fastq"), "rb").read()


def test_reference_decompressor_ignores_the_stream(tmp_path, fq, plain_archive):
    ref = os.path.join(ROOT, "oracle", "_ref", "colord")
    assert os.path.exists(ref), "oracle/_ref/colord is built by build()"
    arc = str(tmp_path / "a.colord")
    run(["compress-ont", "--kmer-spectrum", fq, arc])
    for a, out in ((plain_archive, "p.fastq"), (arc, "k.fastq")):
        subprocess.check_call([ref, "decompress", a, str(tmp_path / out)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert open(str(tmp_path / "p.fastq"), "rb").read() == open(str(tmp_path / "k.fastq"), "rb").read()


def test_an_archive_without_the_option_has_no_spectrum(plain_archive):
    assert "hipkmers" not in AR.read_archive(plain_archive)
    assert "k-mer spectrum" not in run(["info", plain_archive]).stderr
    r = run(["info", "--kmer-spectrum", plain_archive], ok=False)
    assert r.returncode == 1 and "no k-mer spectrum is stored" in r.stderr


@pytest.mark.parametrize("extra", [["--stream-input", "--chunk-bases", "5e5"], ["--gpus", "2", "--gpu-list", "0,0", "--transport", "host"]], ids=["stream_input_chunks", "two_ranks"])
def test_the_same_spectrum_however_the_kmers_reach_the_counter(tmp_path, fq, extra):
    """chunks add their k-mers to one array before the sort; two ranks own disjoint key ranges of one set: sets == 1 and every number the same"""
    arc = str(tmp_path / "x.colord")
    run(["compress-ont", "--kmer-spectrum"] + extra + [fq, arc])
    o, got = printed(arc)
    assert K.same(got, judged("c1_ont_default")) is None, K.same(got, judged("c1_ont_default"))
    assert o["derived"]["estimates"] is True


def test_domains_add_their_sets(tmp_path, fq):
    arc = str(tmp_path / "d.colord")
    run(["compress-ont", "--kmer-spectrum", "--domains", "2", fq, arc])
    o, got = printed(arc, sets=2)
    h = K.hist(got)
    assert got["kmers"] == sum(c * h[c] for c in range(K.EXACT)) + int(got["big_mass"].sum()) == judged("c1_ont_default")["kmers"]      # every read's k-mers, in one domain or the other
    assert got["distinct"] == sum(h) >= judged("c1_ont_default")["distinct"]
    assert o["derived"]["estimates"] is False and not {"valley", "peak", "genome_size"} & set(o["derived"])
    assert "not estimated" in run(["info", "--kmer-spectrum", arc]).stdout


def test_with_a_reference_genome(tmp_path, fq):
    """-G -s: the genome's sequences are a second input of the counter, so its k-mers are in the spectrum: flag bit 0, no estimate"""
    from test_gpu_genome import genome_sequences, readset
    gen = str(tmp_path / "M.bovis-reference.fna")
    open(gen, "wb").write(gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis-reference.fna.gz"), "rb").read())
    arc = str(tmp_path / "g.colord")
    run(["compress-ont", "--kmer-spectrum", "-G", gen, "-s", fq, arc])
    o, got = printed(arc, cfg="c4_ont_genome", flags=1)
    g = golden("c4_ont_genome")
    km = np.concatenate([O.kmer_scan_reads(g.reads, o["k"], o["f"]), O.kmer_scan_reads(readset(genome_sequences(g.spec["genome"])), o["k"], o["f"])])
    want = K.from_kmers(km)
    assert K.same(got, want) is None, K.same(got, want)
    assert o["derived"]["kept_distinct"] == g.p("n_unique") == len(g.kept[0])
    assert o["derived"]["estimates"] is False and "not estimated" in run(["info", "--kmer-spectrum", arc]).stdout
