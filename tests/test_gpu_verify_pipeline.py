"""GPU suite for the opt-in check of the edit scripts (cl_ctx_set_verify / `colord_hip compress-* --verify-scripts`): with it on, the
one-call driver, the chunked compressor (encode lanes included) and the command line rebuild every read from its edit script on the
device (csrc/expand.hip) before coding — and write exactly the bytes they write with it off; the counters equal the input's reads and bases."""
import gzip
import hashlib
import os
import re
import subprocess
import numpy as np
import pytest
from util import golden
from bench import reference_part_bounds
from colord_amd import archive as AR
from test_gpu_stream import params_of, one_call, chunked, even_cuts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")


@pytest.mark.parametrize("cfg,pack_symbols,n_chunks", [("s6m_ont", 1 << 19, 4), ("s5m_hifi", 1 << 20, 2)])
def test_drivers_verify_and_write_the_same_parts(ctx, cfg, pack_symbols, n_chunks):
    from oracle import pyoracle as O
    g = golden(cfg)
    rs = g.reads
    prm = params_of(g)
    packs = reference_part_bounds(np.diff(rs.offsets).astype(np.uint32), pack_symbols)
    assert len(packs) - 1 >= n_chunks
    qm, qual_args = g.p("qual_mode"), None
    if rs.quals is not None and len(rs.quals) and qm != 8:
        d = O.QUAL_DEFAULTS[qm]
        qual_args = (qm, g.p("source"), g.p("level"), tuple(d[0]), tuple(d[1]))
    cuts = even_cuts(len(packs) - 1, n_chunks)
    whole = (rs.n_reads, int(rs.offsets[-1]))
    off_one = one_call(ctx, rs, prm, packs, qual_args)
    off_chunked = chunked(ctx, rs, prm, packs, cuts, qual_args, announce="all")
    ctx.set_verify(True)
    try:
        v0 = ctx.verified()
        on_one = one_call(ctx, rs, prm, packs, qual_args)
        v1 = ctx.verified()
        on_chunked = chunked(ctx, rs, prm, packs, cuts, qual_args, announce="all")     # stage A on the encode lanes
        v2 = ctx.verified()
    finally:
        ctx.set_verify(False)
    assert on_one[:4] == off_one[:4], "one-call driver: parts differ with the check on"
    assert on_chunked[:4] == off_chunked[:4], "chunked compressor: parts differ with the check on"
    assert (v1[0] - v0[0], v1[1] - v0[1]) == whole and (v2[0] - v1[0], v2[1] - v1[1]) == whole
    v3 = ctx.verified()
    one_call(ctx, rs, prm, packs, qual_args)
    assert ctx.verified() == v3, "the check ran although it was switched off"


def _streams(path):
    return {name: [(m, hashlib.sha256(p).hexdigest()) for m, p in s.parts] for name, s in AR.read_archive(path).items() if name != "info"}


@pytest.mark.skipif(not os.path.exists(CLI), reason="needs colord_amd/colord_hip")
@pytest.mark.parametrize("extra", [[], ["--stream-input"], ["-G", "GENOME", "-s"], ["--gpus", "2", "--gpu-list", "0,0", "--transport", "host"]], ids=["plain", "stream_input", "genome", "two_ranks"])
def test_cli_verify_scripts_changes_no_byte(tmp_path, extra):
    fq, gen = str(tmp_path / "M.bovis.fastq"), str(tmp_path / "M.bovis-reference.fna")
    raw = gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis.fastq.gz"), "rb").read()
    open(fq, "wb").write(raw)
    n_reads = raw.count(b"\n") // 4
    if "-G" in extra:
        open(gen, "wb").write(gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis-reference.fna.gz"), "rb").read())
        extra = [gen if x == "GENOME" else x for x in extra]
    plain, checked = str(tmp_path / "off.colord"), str(tmp_path / "on.colord")
    subprocess.check_call([CLI, "compress-ont"] + extra + [fq, plain])
    r = subprocess.run([CLI, "compress-ont", "--verify-scripts", "-v"] + extra + [fq, checked], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert _streams(checked) == _streams(plain)
    counts = [int(m) for m in re.findall(r"# edit scripts verified[^:]*: (\d+) reads", r.stderr)]
    assert counts and sum(counts) == n_reads, r.stderr
