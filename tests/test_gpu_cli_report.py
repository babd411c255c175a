"""GPU suite of `colord_hip compress-* --report`: the archive stores a `hipreport` stream counted on the device from the input;
`info --report --json` prints it; `decompress` / `check` recompute its output side from what they decode.  The judge is tests/report_ref.py
over the input FASTQ.  Input: tests/data/M.bovis.fastq.gz (100 reads); the off path against the reference-written golden archive of its
first 24 reads."""
import gzip
import hashlib
import json
import os
import subprocess
import numpy as np
import pytest
from colord_amd import archive as AR
import digest_ref as R
import report_ref as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
OK = "content report: ok"


def run(args, ok=True):
    r = subprocess.run([CLI] + args, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rp_in") / "M.bovis.fastq")
    open(path, "wb").write(gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis.fastq.gz"), "rb").read())
    return path


@pytest.fixture(scope="module")
def records(fq):
    """(codes, input quality bytes) of the input"""
    recs = R.parse_fastq(fq)
    return [r[1] for r in recs], [(r[2].astype(np.int64) + 33).astype(np.uint8) for r in recs]


def stored(path):
    arc = AR.read_archive(path)
    assert "hipreport" in arc and len(arc["hipreport"].parts) == 1
    meta, payload = arc["hipreport"].parts[0]
    assert meta == 0
    return P.unpack_hipreport(payload), payload


def streams(path, skip=("info", "hipreport")):
    return {n: [(m, hashlib.sha256(p).hexdigest()) for m, p in s.parts] for n, s in AR.read_archive(path).items() if n not in skip}


def same_as(got, ref):
    return P.same(got, ref) is None and (got["n50"], got["n90"]) == (ref["n50"], ref["n90"])


@pytest.mark.parametrize("extra,mode,T,D", [([], "4-avg", None, None), (["-q", "org"], "org", None, None), (["-q", "2-fix", "-D", "5,20"], "2-fix", None, [5, 20]), (["-q", "avg"], "avg", None, None),
                                            (["-q", "5-avg", "-T", "5,12,30,60"], "5-avg", [5, 12, 30, 60], None), (["-q", "none"], "none", None, None)],
                         ids=["default_4-avg", "org", "2-fix_D", "avg", "5-avg_T", "none"])
def test_the_report_is_stored_printed_and_confirmed(tmp_path, fq, records, extra, mode, T, D):
    arc, out = str(tmp_path / "a.colord"), str(tmp_path / "o.fastq")
    run(["compress-ont", "--report"] + extra + [fq, arc])
    ref = P.report(records[0], records[1], mode, T, D)
    st, payload = stored(arc)
    assert same_as(st, ref), P.same(st, ref)
    assert payload == P.pack_hipreport(ref)
    assert "content report: 100 reads, %d bases, N50 %d" % (ref["bases"], ref["n50"]) in run(["info", arc]).stderr
    o = json.loads(run(["info", "--report", "--json", arc]).stdout)
    assert o["reads"] == 100 and o["base_count"] == [int(x) for x in ref["base_count"]] and o["has_qual"] == ref["has_qual"]
    if ref["has_qual"]:
        assert sorted(map(tuple, o["q_joint"])) == [(i, j, int(ref["q_joint"][i, j])) for i in range(96) for j in range(96) if ref["q_joint"][i, j]]
    assert OK in run(["decompress", arc, out]).stderr
    # the report of the FASTQ that came back: its OUT marginal is the stored one's
    back = R.parse_fastq(out)
    if ref["has_qual"]:
        hist = np.bincount(np.concatenate([r[2] for r in back]).astype(np.int64), minlength=96).astype(np.uint64)
        assert np.array_equal(hist, P.out_marginal(st))
    assert OK in run(["check", arc]).stdout


@pytest.fixture(scope="module")
def baseline(tmp_path_factory, fq):
    arc = str(tmp_path_factory.mktemp("rp_base") / "base.colord")
    run(["compress-ont", "--report", fq, arc])
    return stored(arc)[1]


@pytest.mark.parametrize("extra", [["--part-symbols", "4096"], ["--chunk-bases", "1e5"], ["--stream-input", "--chunk-bases", "1e5"], ["--domains", "2"],
                                   ["--gpus", "2", "--gpu-list", "0,0", "--transport", "host"]], ids=["part_symbols", "chunks", "stream_input", "domains", "two_ranks"])
def test_the_stored_report_is_the_same_however_the_input_is_cut(tmp_path, fq, records, baseline, extra):
    arc, out = str(tmp_path / "x.colord"), str(tmp_path / "o.fastq")
    run(["compress-ont", "--report"] + extra + [fq, arc])
    assert stored(arc)[1] == baseline == P.pack_hipreport(P.report(records[0], records[1], "4-avg"))
    assert OK in run(["decompress", arc, out]).stderr
    assert OK in run(["check", arc]).stdout


def test_with_a_stored_reference_genome(tmp_path, fq, records, baseline):
    """-G -s: the genome's pseudo reads are reference reads, not content"""
    gen = str(tmp_path / "M.bovis-reference.fna")
    open(gen, "wb").write(gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis-reference.fna.gz"), "rb").read())
    arc, out = str(tmp_path / "g.colord"), str(tmp_path / "o.fastq")
    run(["compress-ont", "--report", "-G", gen, "-s", fq, arc])
    assert stored(arc)[1] == baseline
    assert OK in run(["decompress", arc, out]).stderr


def test_the_device_decoder_is_checked_too(tmp_path, fq, baseline):
    """--qual-domain-symbols + --gpu: the quality lines come out of k_qual_decode and are counted where they are handed to the writer"""
    arc, host, dev = str(tmp_path / "q.colord"), str(tmp_path / "h.fastq"), str(tmp_path / "d.fastq")
    run(["compress-ont", "--report", "--part-symbols", "4096", "--qual-domain-symbols", "60000", fq, arc])
    assert stored(arc)[1] == baseline
    r = run(["decompress", "--gpu", "0", arc, dev])
    assert OK in r.stderr and "quality stream decoded on GPU 0" in r.stderr
    assert OK in run(["decompress", arc, host]).stderr
    assert open(host, "rb").read() == open(dev, "rb").read()
    assert OK in run(["check", "--gpu", "0", arc]).stdout


def test_without_the_option_every_byte_is_the_reference_archives(tmp_path, fq):
    """the first 24 reads, -q 4-avg -p balanced: without --report every stream but `info` is the reference-written golden archive's (what the
    parent wrote); with it every stream but `info` and `hipreport` is, too"""
    lines = open(fq, "rb").read().split(b"\n")
    src = str(tmp_path / "b24.fastq")
    open(src, "wb").write(b"\n".join(lines[:96]) + b"\n")
    plain, rep = str(tmp_path / "plain.colord"), str(tmp_path / "rep.colord")
    run(["compress-ont", "-q", "4-avg", "-p", "balanced", src, plain])
    run(["compress-ont", "-q", "4-avg", "-p", "balanced", "--report", src, rep])
    gold = streams(os.path.join(ROOT, "tests", "golden", "archives", "bovis24_q_4-avg_balanced.colord"))
    assert streams(plain) == gold == streams(rep)
    assert "hipreport" not in AR.read_archive(plain) and set(AR.read_archive(rep)) == set(AR.read_archive(plain)) | {"hipreport"}
    assert "content report" not in run(["decompress", plain, str(tmp_path / "o.fastq")]).stderr


def test_fasta_input_has_no_quality_part(tmp_path, fq, records):
    lines = open(fq, "rb").read().split(b"\n")
    src = str(tmp_path / "in.fasta")
    with open(src, "wb") as f:
        for i in range(0, len(lines) - 3, 4):
            f.write(b">" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n")
    arc = str(tmp_path / "n.colord")
    run(["compress-ont", "--report", src, arc])
    st, payload = stored(arc)
    assert payload == P.pack_hipreport(P.report(records[0])) and st["has_qual"] == 0
    assert OK in run(["decompress", arc, str(tmp_path / "o.fa")]).stderr


def test_a_fix_value_the_report_cannot_count_is_refused(tmp_path, fq):
    arc = str(tmp_path / "x.colord")
    r = run(["compress-ont", "--report", "-q", "2-fix", "-D", "5,120", fq, arc], ok=False)
    assert "--report: a -D value above 95" in r.stderr and not os.path.exists(arc)
