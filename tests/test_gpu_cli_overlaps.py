"""GPU suite of `colord_hip compress-* --overlaps`: the archive stores a `hipoverlaps` stream made on the device from the tuple
streams; `info --overlaps [--min-block N] [--names]` prints it as PAF.  The input is the synthetic set of the golden s6m_ont (374 reads of a
200-kb genome, `compress-ont`), whose tuple streams and acceptor decisions the unmodified reference recorded: the judge (tests/overlaps_ref.py)
walks those, and the library's own pipeline (cl_compress_shard with cl_ctx_set_overlaps) must have kept the same records."""
import hashlib
import os
import subprocess
import numpy as np
import pytest
from colord_amd import archive as AR
from colord_amd.fastq import write_fastq
from util import golden
import overlaps_ref as OR
from test_edits_cpu import golden_refs
from test_gpu_stream import params_of, one_call
from test_gpu_encode import sparse_g

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
CFG = "s6m_ont"


def run(args, ok=True):
    r = subprocess.run([CLI] + args, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ov_in") / "s6m.fastq")
    write_fastq(path, golden(CFG).reads)
    return path


@pytest.fixture(scope="module")
def want():
    g = golden(CFG)
    rs = g.reads
    table = np.nonzero(g.accept[len(g.accept) - rs.n_reads:].astype(bool) & ~rs.has_n())[0].astype(np.uint32)
    return OR.records([e[2] for e in g.es], golden_refs(CFG), 0, table)


@pytest.fixture(scope="module")
def archives(tmp_path_factory, fq):
    d = tmp_path_factory.mktemp("ov_arc")
    plain, with_ov = str(d / "plain.colord"), str(d / "ov.colord")
    run(["compress-ont", fq, plain])
    run(["compress-ont", "--overlaps", fq, with_ov])
    return plain, with_ov


def streams(path, skip=("info", "hipoverlaps")):
    return {n: [(m, hashlib.sha256(p).hexdigest()) for m, p in s.parts] for n, s in AR.read_archive(path).items() if n not in skip}


def test_the_records_are_stored_and_printed_and_no_other_byte_changes(ctx, tmp_path, fq, archives, want):
    plain, arc = archives
    a = AR.read_archive(arc)
    assert "hipoverlaps" in a and len(a["hipoverlaps"].parts) == 1
    assert a["hipoverlaps"].parts[0][1] == OR.pack_hipoverlaps(want) and len(want) > 300
    g = golden(CFG)                                                           # the library's own records of the same input
    ctx.set_overlaps(True)
    try:
        one_call(ctx, g.reads, dict(params_of(g), sparse_g=sparse_g(g)), [int(x) for x in g.reads.pack_bounds()], None)
        lib = ctx.overlaps()
    finally:
        ctx.set_overlaps(False)
    ctx.set_overlaps(True); ctx.set_overlaps(False)                             # (nothing is left on the shared context)
    assert np.array_equal(lib, want)
    lines = run(["info", "--overlaps", arc]).stdout.splitlines()
    assert lines == OR.paf_lines(lib)
    assert streams(arc) == streams(plain)                                       # every stream but `info` and `hipoverlaps`
    assert "hipoverlaps" not in AR.read_archive(plain) and set(a) == set(AR.read_archive(plain)) | {"hipoverlaps"}
    assert "overlaps: %d records" % len(want) in run(["info", arc]).stderr and "overlaps" not in run(["info", plain]).stderr
    out = str(tmp_path / "o.fastq")
    run(["decompress", arc, out])                                             # the decoders ignore the stream
    assert open(out, "rb").read() == open(fq, "rb").read()
    run(["check", arc])


def test_names_and_min_block(archives, want):
    _, arc = archives
    ids = [h.decode().split()[0] for h in golden(CFG).reads.headers]
    assert ids[5] == "read_5"
    assert run(["info", "--overlaps", "--names", arc]).stdout.splitlines() == OR.paf_lines(want, names=ids)
    blocks = sorted(OR.block(r) for r in want)
    mid = blocks[len(blocks) // 2]
    got = run(["info", "--overlaps", "--min-block", str(mid), arc]).stdout.splitlines()
    assert got == OR.paf_lines(want, min_block=mid) and 0 < len(got) < len(want)
    assert run(["info", "--overlaps", "--min-block", str(blocks[-1] + 1), "--names", arc]).stdout == ""


@pytest.mark.parametrize("extra", [["--part-symbols", "65536"], ["--stream-input", "--chunk-bases", "1e6"]], ids=["part_symbols", "stream_input_chunks"])
def test_the_same_records_however_the_input_is_cut(tmp_path, fq, want, extra):
    arc = str(tmp_path / "x.colord")
    run(["compress-ont", "--overlaps"] + extra + [fq, arc])
    assert AR.read_archive(arc)["hipoverlaps"].parts[0][1] == OR.pack_hipoverlaps(want)


@pytest.mark.parametrize("extra,text", [(["--gpus", "2", "--gpu-list", "0,0", "--transport", "host"], "--overlaps is not available with --gpus > 1"),
                                        (["--domains", "2"], "--overlaps is not available with --domains > 1"), (["-G", "genome.fa"], "--overlaps is not available with -G")],
                         ids=["gpus", "domains", "genome"])
def test_refused_combinations(tmp_path, fq, extra, text):
    arc = str(tmp_path / "r.colord")
    r = run(["compress-ont", "--overlaps"] + extra + [fq, arc], ok=False)
    assert r.returncode == 1 and text in r.stderr
    assert not os.path.exists(arc)
