"""GPU suite of `colord_hip compress-* --edit-profile`: the archive stores a `hipedits` stream counted on the device from the tuple
streams; `info --edit-profile --json` prints it.  The judge is tests/edits_ref.py over the tuple streams the unmodified reference made of the same
input with the same parameters (golden es.bin of c1_ont_default: tests/data/M.bovis.fastq.gz, 100 reads, `compress-ont`; c4_ont_genome with -G -s)."""
import gzip
import hashlib
import json
import os
import subprocess
import numpy as np
import pytest
from colord_amd import archive as AR
import edits_ref as E
from test_edits_cpu import judged

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")


def run(args, ok=True):
    r = subprocess.run([CLI] + args, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ed_in") / "M.bovis.fastq")
    open(path, "wb").write(gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis.fastq.gz"), "rb").read())
    return path


def printed(arc):
    """the profile as `info --edit-profile --json` prints it, and the stored payload"""
    a = AR.read_archive(arc)
    assert "hipedits" in a and len(a["hipedits"].parts) == 1 and a["hipedits"].parts[0][0] == 0
    payload = a["hipedits"].parts[0][1]
    o = json.loads(run(["info", "--edit-profile", "--json", arc]).stdout)
    got = {k: (np.array(o[k], np.uint64) if s else o[k]) for k, s in E.FIELDS}
    assert E.pack_hipedits(got) == payload and len(payload) == 8 + 8 * E.WORDS
    return got


def streams(path, skip=("info", "hipedits")):
    return {n: [(m, hashlib.sha256(p).hexdigest()) for m, p in s.parts] for n, s in AR.read_archive(path).items() if n not in skip}


@pytest.fixture(scope="module")
def plain_archive(tmp_path_factory, fq):
    arc = str(tmp_path_factory.mktemp("ed_base") / "plain.colord")
    run(["compress-ont", fq, arc])
    return arc


def test_the_profile_is_stored_and_printed_and_no_other_byte_changes(tmp_path, fq, plain_archive):
    arc = str(tmp_path / "a.colord")
    run(["compress-ont", "--edit-profile", fq, arc])
    want = judged("c1_ont_default")
    got = printed(arc)
    assert E.same(got, want) is None, E.same(got, want)
    assert streams(arc) == streams(plain_archive)                               # every stream but `info` and `hipedits`
    assert "hipedits" not in AR.read_archive(plain_archive) and set(AR.read_archive(arc)) == set(AR.read_archive(plain_archive)) | {"hipedits"}
    i = run(["info", arc])
    assert "edit profile: %d of 100 reads coded with an edit script" % int(want["kind_reads"][2]) in i.stderr
    assert "edit profile" not in run(["info", plain_archive]).stderr
    t = run(["info", "--edit-profile", arc]).stdout
    assert "not a per-read error rate" in t and "reads: 100\n" in t
    out = str(tmp_path / "o.fastq")
    run(["decompress", arc, out])                                             # the decoders ignore the stream
    run(["decompress", plain_archive, str(tmp_path / "p.fastq")])
    assert open(out, "rb").read() == open(str(tmp_path / "p.fastq"), "rb").read()


@pytest.mark.parametrize("extra", [["--part-symbols", "65536"], ["--stream-input"], ["--chunk-bases", "1e5"], ["--stream-input", "--chunk-bases", "1e5", "--part-symbols", "65536"]],
                         ids=["part_symbols", "stream_input", "chunks", "all_three"])
def test_the_same_numbers_however_the_input_is_cut(tmp_path, fq, extra):
    arc = str(tmp_path / "x.colord")
    run(["compress-ont", "--edit-profile"] + extra + [fq, arc])
    got = printed(arc)
    assert E.same(got, judged("c1_ont_default")) is None, E.same(got, judged("c1_ont_default"))


def test_with_a_stored_reference_genome(tmp_path, fq):
    """-G -s: the profile against the genome's pseudo reads and the reads before"""
    gen = str(tmp_path / "M.bovis-reference.fna")
    open(gen, "wb").write(gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis-reference.fna.gz"), "rb").read())
    arc = str(tmp_path / "g.colord")
    run(["compress-ont", "--edit-profile", "-G", gen, "-s", fq, arc])
    got = printed(arc)
    assert E.same(got, judged("c4_ont_genome")) is None, E.same(got, judged("c4_ont_genome"))


@pytest.mark.parametrize("extra", [["--domains", "2"], ["--gpus", "2", "--gpu-list", "0,0", "--transport", "host"]], ids=["domains", "two_ranks"])
def test_domains_add_their_parts(tmp_path, fq, extra):
    """every domain has reference reads of its own, so only what does not depend on them is the same: the reads, the bases, the invariants"""
    arc = str(tmp_path / "d.colord")
    run(["compress-ont", "--edit-profile"] + extra + [fq, arc])
    got = printed(arc)
    want = judged("c1_ont_default")
    assert got["reads"] == want["reads"] == 100 and got["bases"] == want["bases"]
    assert E.invariants(got) == []
    assert int(got["kind_reads"][1]) == int(want["kind_reads"][1])              # (a read with Ns is coded plain wherever it lies)
