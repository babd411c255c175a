"""GPU suite of `colord_hip compress-* --digest-values`: the archive stores a fourth digest, qual-values, made on the
device from the input qualities; `decompress` / `check` recompute it from the quality bytes they hand to the writer.  The judge is
tests/qual_values_ref.py over the quality lines of the FASTQ that comes back.  Input: tests/data/M.bovis.fastq.gz (100 reads)."""
import gzip
import hashlib
import os
import subprocess
import pytest
from colord_amd import archive as AR
import qual_values_ref as V
from test_qual_values_cpu import parse_check4

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
FOUR = "content digest: ok (dna, qual, qual-values, header)"


def run(args, ok=True):
    r = subprocess.run([CLI] + args, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("dv_in") / "M.bovis.fastq")
    open(path, "wb").write(gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis.fastq.gz"), "rb").read())
    return path


def stored(path):
    arc = AR.read_archive(path)
    assert "hipdigest" in arc and len(arc["hipdigest"].parts) == 1
    meta, payload = arc["hipdigest"].parts[0]
    assert meta == 0
    return V.unpack_hipdigest_any(payload), len(payload)


def streams(path, skip=("info",)):
    return {n: [(m, hashlib.sha256(p).hexdigest()) for m, p in s.parts] for n, s in AR.read_archive(path).items() if n not in skip}


@pytest.mark.parametrize("extra", [[], ["-q", "org"], ["-q", "2-fix", "-D", "5,20"], ["-q", "avg"]], ids=["default_4-avg", "org", "2-fix_D", "avg"])
def test_four_digests_are_stored_and_confirmed(tmp_path, fq, extra):
    arc, out = str(tmp_path / "a.colord"), str(tmp_path / "o.fastq")
    run(["compress-ont", "--digest-values"] + extra + [fq, arc])
    st, size = stored(arc)
    assert size == 104 and st["version"] == 2 and st["flags"] == 15
    i = run(["info", arc])
    assert i.stderr.count("content digest: ") == 4 and "content digest: qual-values reads=100 " in i.stderr
    r = run(["decompress", arc, out])
    assert FOUR in r.stderr
    # the digest of the quality lines that came back, by the Python reference, is the stored one
    assert V.digest_fastq_quality_lines(out) == st["qval"]
    c = run(["check", arc])
    got = parse_check4(c.stdout)
    assert FOUR in c.stdout and got["qual-values"] == got["stored qual-values"] == st["qval"]


@pytest.fixture(scope="module")
def baseline(tmp_path_factory, fq):
    arc = str(tmp_path_factory.mktemp("dv_base") / "base.colord")
    run(["compress-ont", "--digest-values", fq, arc])
    return stored(arc)[0]


@pytest.mark.parametrize("extra", [["--part-symbols", "4096"], ["--chunk-bases", "1e5"], ["--stream-input", "--chunk-bases", "1e5"], ["--domains", "2"],
                                   ["--gpus", "2", "--gpu-list", "0,0", "--transport", "host"]], ids=["part_symbols", "chunks", "stream_input", "domains", "two_ranks"])
def test_the_stored_digests_are_the_same_however_the_input_is_cut(tmp_path, fq, baseline, extra):
    arc, out = str(tmp_path / "x.colord"), str(tmp_path / "o.fastq")
    run(["compress-ont", "--digest-values"] + extra + [fq, arc])
    st, size = stored(arc)
    assert size == 104 and st == baseline
    assert FOUR in run(["decompress", arc, out]).stderr


def test_the_device_decoder_is_checked_against_the_integer_values(tmp_path, fq, baseline):
    """--qual-domain-symbols + --gpu: the quality lines come out of k_qual_decode's double arithmetic and are digested where they are handed to the
    writer; the stored digest was made from the input by integers"""
    arc, host, dev = str(tmp_path / "q.colord"), str(tmp_path / "h.fastq"), str(tmp_path / "d.fastq")
    run(["compress-ont", "--digest-values", "--part-symbols", "4096", "--qual-domain-symbols", "60000", fq, arc])
    st, _ = stored(arc)
    assert st["qval"] == baseline["qval"] and st["dna"] == baseline["dna"]
    r = run(["decompress", "--gpu", "0", arc, dev])
    assert FOUR in r.stderr and "quality stream decoded on GPU 0" in r.stderr
    assert FOUR in run(["decompress", arc, host]).stderr
    assert open(host, "rb").read() == open(dev, "rb").read()
    c = run(["check", "--gpu", "0", arc])
    assert FOUR in c.stdout and parse_check4(c.stdout)["qual-values"] == st["qval"]


def test_without_the_option_nothing_changes(tmp_path, fq, baseline):
    plain, dig, val = (str(tmp_path / x) for x in ("plain.colord", "dig.colord", "val.colord"))
    run(["compress-ont", fq, plain]); run(["compress-ont", "--digest", fq, dig]); run(["compress-ont", "--digest-values", fq, val])
    a, b, c = streams(plain, ("info", "hipdigest")), streams(dig, ("info", "hipdigest")), streams(val, ("info", "hipdigest"))
    assert a == b == c
    assert "hipdigest" not in AR.read_archive(plain)
    st, size = stored(dig)
    assert size == 80 and st["version"] == 1 and st["flags"] == 7 and st["qval"] is None
    for k in ("dna", "qual", "header"):
        assert st[k] == baseline[k]
    r = run(["decompress", dig, str(tmp_path / "o.fastq")])
    assert "content digest: ok (dna, qual, header)" in r.stderr


@pytest.mark.parametrize("args,why", [(["-q", "none"], "-q none"), (["--fasta"], "no qualities")])
def test_without_a_coded_quality_stream_it_is_plain_digest(tmp_path, fq, args, why):
    src = fq
    if args == ["--fasta"]:
        lines = open(fq, "rb").read().split(b"\n")
        src = str(tmp_path / "in.fasta")
        with open(src, "wb") as f:
            for i in range(0, len(lines) - 3, 4):
                f.write(b">" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n")
        args = []
    arc = str(tmp_path / "n.colord")
    r = run(["compress-ont", "--digest-values", "-v"] + args + [src, arc])
    assert "--digest-values" in r.stderr and why in r.stderr
    st, size = stored(arc)
    assert size == 80 and st["version"] == 1 and not st["flags"] & 8
    assert "content digest: ok" in run(["decompress", arc, str(tmp_path / "o.fx")]).stderr
