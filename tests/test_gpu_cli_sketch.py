"""GPU suite of `colord_hip compress-* --sketch` and `colord_hip dist`: the archive stores a `hipsketch` stream made on the device
from the sorted k-mers of pass 1; `info --sketch --json` prints it, `dist` compares archives by it.  The judge is tests/sketch_ref.py over the
k-mers the oracle scans from the same reads (tests/data/M.bovis.fastq.gz, 100 reads, `compress-ont`: the parameters of c1_ont_default; with
-G -s those of c4_ont_genome)."""
import functools
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
import sketch_ref as S
from test_kspec_cpu import golden_kmers
from test_sketch_cpu import printed as sketch_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
FIRST = 60


def run(args, ok=True):
    r = subprocess.run([CLI] + args, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("sk_in") / "M.bovis.fastq")
    open(path, "wb").write(gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis.fastq.gz"), "rb").read())
    return path


@pytest.fixture(scope="module")
def fq60(tmp_path_factory, fq):
    """the first 60 records of the input"""
    lines = open(fq, "rb").read().split(b"\n")
    assert all(lines[4 * i].startswith(b"@") and lines[4 * i + 2].startswith(b"+") for i in range(100))
    path = str(tmp_path_factory.mktemp("sk_in60") / "first60.fastq")
    open(path, "wb").write(b"\n".join(lines[:4 * FIRST]) + b"\n")
    return path


@functools.lru_cache(maxsize=None)
def kmers_of_the_first_60():
    g = golden("c1_ont_default")
    return np.concatenate([O.kmer_scan(g.reads.read(i), g.p("k"), g.p("f")) for i in range(FIRST)])


def printed(arc, cfg="c1_ont_default", sets=1, flags=0, size=10000, m=2):
    """the JSON of `info --sketch --json` and its sketch; the header states the parameters of cfg, the stored payload is the judge's packing of what is printed"""
    a = AR.read_archive(arc)
    assert "hipsketch" in a and len(a["hipsketch"].parts) == 1 and a["hipsketch"].parts[0][0] == 0
    payload = a["hipsketch"].parts[0][1]
    o = json.loads(run(["info", "--sketch", "--json", arc]).stdout)
    g = golden(cfg)
    assert [o[x] for x in ("version", "flags", "k", "f", "min_count", "size", "sets")] == [1, flags, g.p("k"), g.p("f"), m, size, sets]
    got = sketch_of(o)
    assert S.pack(got, o["k"], o["f"], sets=sets, flags=flags) == payload
    return o, got, payload


def streams(path, skip=("info", "hipsketch")):
    return {n: [(m, hashlib.sha256(p).hexdigest()) for m, p in s.parts] for n, s in AR.read_archive(path).items() if n not in skip}


@pytest.fixture(scope="module")
def plain_archive(tmp_path_factory, fq):
    arc = str(tmp_path_factory.mktemp("sk_base") / "plain.colord")
    run(["compress-ont", fq, arc])
    return arc


def test_the_sketch_is_stored_and_printed_and_no_other_byte_changes(tmp_path, fq, plain_archive):
    arc = str(tmp_path / "a.colord")
    run(["compress-ont", "--sketch", "--sketch-size", "500", fq, arc])
    want = S.from_kmers(golden_kmers("c1_ont_default"), 500, 2)
    o, got, payload = printed(arc, size=500)
    assert S.same(got, want) is None, S.same(got, want)
    assert payload == S.pack(want, o["k"], o["f"]) and len(payload) == 48 + 16 * 500
    assert o["complete"] is False and o["qualifying"] == 2522
    assert streams(arc) == streams(plain_archive)                               # every stream but `info` and `hipsketch`
    assert "hipsketch" not in AR.read_archive(plain_archive) and set(AR.read_archive(arc)) == set(AR.read_archive(plain_archive)) | {"hipsketch"}
    assert "k-mer sketch: 500 of 2522 qualifying k-mers" in run(["info", arc]).stderr
    assert "hash sample" in run(["info", "--sketch", arc]).stdout
    out = str(tmp_path / "o.fastq")
    run(["decompress", arc, out])                                               # the decoders ignore the stream
    run(["decompress", plain_archive, str(tmp_path / "p.fastq")])
    assert open(out, "rb").read() == open(str(tmp_path / "p.fastq"), "rb").read()
    ref = os.path.join(ROOT, "oracle", "_ref", "colord")
    assert os.path.exists(ref), "oracle/_ref/colord is built by build()"
    subprocess.check_call([ref, "decompress", arc, str(tmp_path / "r.fastq")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert open(str(tmp_path / "r.fastq"), "rb").read() == open(out, "rb").read()


def test_the_default_size_gives_a_complete_sketch(tmp_path, fq):
    arc = str(tmp_path / "a.colord")
    run(["compress-ont", "--sketch", fq, arc])
    o, got, _ = printed(arc)
    want = S.from_kmers(golden_kmers("c1_ont_default"), 10000, 2)
    assert S.same(got, want) is None and o["complete"] is True and o["n"] == o["qualifying"] == 2522
    d = json.loads(run(["dist", "--json", arc, arc]).stdout)
    assert (d["jaccard"], d["distance"], d["shared"], d["compared"]) == (1.0, 0.0, 2522, 2522)


def test_an_archive_without_the_option_has_no_sketch(plain_archive):
    assert "k-mer sketch" not in run(["info", plain_archive]).stderr
    r = run(["info", "--sketch", plain_archive], ok=False)
    assert r.returncode == 1 and "no k-mer sketch is stored" in r.stderr and r.stdout == ""
    r = run(["dist", plain_archive, plain_archive], ok=False)
    assert r.returncode == 1 and "no k-mer sketch is stored" in r.stderr and plain_archive in r.stderr and r.stdout == ""


@pytest.mark.parametrize("extra", [["--stream-input", "--chunk-bases", "5e5"], ["--gpus", "2", "--gpu-list", "0,0", "--transport", "host"]], ids=["stream_input_chunks", "two_ranks"])
def test_the_same_bytes_however_the_kmers_reach_the_counter(tmp_path, fq, extra):
    """chunks add their k-mers to one array before the sort; two ranks own disjoint key ranges of one set: sets == 1 and the payload byte for byte"""
    arc = str(tmp_path / "x.colord")
    run(["compress-ont", "--sketch", "--sketch-size", "500"] + extra + [fq, arc])
    o, got, payload = printed(arc, size=500)
    assert payload == S.pack(S.from_kmers(golden_kmers("c1_ont_default"), 500, 2), o["k"], o["f"])


def test_domains_merge_their_sets(tmp_path, fq):
    arc = str(tmp_path / "d.colord")
    run(["compress-ont", "--sketch", "--sketch-size", "500", "--domains", "2", fq, arc])
    o, got, _ = printed(arc, sets=2, size=500)
    assert len(got["hash"]) == 500 and np.all(got["hash"][1:] > got["hash"][:-1])
    keys, counts = np.unique(golden_kmers("c1_ont_default"), return_counts=True)
    km = S.unhash(got["hash"])
    at = np.searchsorted(keys, km)
    assert np.array_equal(keys[np.minimum(at, len(keys) - 1)], km)              # each is a hash of an input k-mer
    assert np.all(got["count"] <= counts[at].astype(np.uint64)) and np.all(got["count"] >= 2)     # (a domain holds some of its occurrences, at least min_count)
    assert o["qualifying"] >= 500
    assert "per set" in run(["info", "--sketch", arc]).stdout


def test_with_a_reference_genome(tmp_path, fq):
    """-G -s: the genome's sequences are a second input of the counter, so its k-mers are in the sketch: flag bit 0"""
    from test_gpu_genome import genome_sequences, readset
    gen = str(tmp_path / "M.bovis-reference.fna")
    open(gen, "wb").write(gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis-reference.fna.gz"), "rb").read())
    arc = str(tmp_path / "g.colord")
    run(["compress-ont", "--sketch", "--sketch-size", "500", "-G", gen, "-s", fq, arc])
    o, got, _ = printed(arc, cfg="c4_ont_genome", flags=1, size=500)
    g = golden("c4_ont_genome")
    km = np.concatenate([O.kmer_scan_reads(g.reads, o["k"], o["f"]), O.kmer_scan_reads(readset(genome_sequences(g.spec["genome"])), o["k"], o["f"])])
    want = S.from_kmers(km, 500, 2)
    assert S.same(got, want) is None, S.same(got, want)
    assert "reference genome counted too: yes" in run(["info", "--sketch", arc]).stdout


@pytest.mark.parametrize("size,m", [(100000, 1), (10000, 2), (500, 1), (500, 2)], ids=["complete_m1", "complete_m2", "size500_m1", "size500_m2"])
def test_dist_between_the_input_and_its_first_60_reads(tmp_path, fq, fq60, size, m):
    a, b = str(tmp_path / "all.colord"), str(tmp_path / "first60.colord")
    opts = ["--sketch", "--sketch-size", str(size), "--sketch-min-count", str(m)]
    run(["compress-ont"] + opts + [fq, a])
    run(["compress-ont"] + opts + [fq60, b])
    wa, wb = S.from_kmers(golden_kmers("c1_ont_default"), size, m), S.from_kmers(kmers_of_the_first_60(), size, m)
    _, ga, _ = printed(a, size=size, m=m)
    _, gb, _ = printed(b, size=size, m=m)
    assert S.same(ga, wa) is None and S.same(gb, wb) is None
    want = S.dist(wa, wb, 20)
    assert 0 < want["shared"] < want["compared"]                                # not vacuous
    if size > 500:                                                              # both complete: the exact Jaccard index of the two qualifying sets
        A, B = set(wa["hash"].tolist()), set(wb["hash"].tolist())
        assert (want["shared"], want["compared"]) == (len(A & B), len(A | B)) and len(wa["hash"]) == wa["qualifying"] and len(wb["hash"]) == wb["qualifying"]
    else:
        assert want["compared"] == 500
    r = run(["dist", "--json", a, b])
    o = json.loads(r.stdout)
    for key in ("shared", "compared", "in_a", "in_b"):
        assert o[key] == want[key], (key, o[key], want[key])
    for key in ("jaccard", "containment_of_a", "containment_of_b", "distance"):
        assert abs(o[key] - want[key]) <= 1e-12 * abs(want[key]), (key, o[key], want[key])
    assert o["jaccard"] == want["shared"] / want["compared"] and r.stderr == ""
    same = json.loads(run(["dist", "--json", a, a]).stdout)
    assert (same["jaccard"], same["distance"]) == (1.0, 0.0)
