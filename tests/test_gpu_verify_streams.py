"""GPU suite for the opt-in check of the coded parts (cl_ctx_set_verify_streams / `colord_hip compress-* --verify-streams`): with it on, the
DNA and quality coders of the one-call driver, the chunked compressor and the command line decode every coded part on the device against
the intervals its models gave (k_range_check, csrc/rc_check.hpp) — and write exactly the bytes they write with it off; the counters equal
the parts and bytes returned; with it off nothing is counted and nothing launched."""
import gzip
import hashlib
import os
import re
import subprocess
import sys
import numpy as np
import pytest
from util import golden
from bench import reference_part_bounds
from colord_amd import archive as AR
from test_gpu_stream import params_of, one_call, chunked, even_cuts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")


def _delta(a, b):
    return tuple(y - x for x, y in zip(a, b))


@pytest.mark.parametrize("cfg,pack_symbols,n_chunks", [("s6m_ont", 1 << 16, 4), ("s5m_hifi", 1 << 20, 2), ("c3_clr_ratio", 1 << 17, 3)])
def test_drivers_verify_streams_and_write_the_same_parts(ctx, cfg, pack_symbols, n_chunks):
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
    off_one = one_call(ctx, rs, prm, packs, qual_args)
    off_chunked = chunked(ctx, rs, prm, packs, cuts, qual_args, announce="all")
    ctx.set_verify_streams(True)
    ctx.lib.cl_ctx_set_timing(ctx.h, 1)
    try:
        ctx.kernel_times()
        v0 = ctx.verified_streams()
        on_one = one_call(ctx, rs, prm, packs, qual_args)
        v1 = ctx.verified_streams()
        launches_on = ctx.kernel_times().get("k_range_check", (0.0, 0))[1]
        ctx.lib.cl_ctx_set_timing(ctx.h, 0)
        on_chunked = chunked(ctx, rs, prm, packs, cuts, qual_args, announce="all")
        v2 = ctx.verified_streams()
        ctx.set_verify_streams(False)
        ctx.lib.cl_ctx_set_timing(ctx.h, 1)
        ctx.kernel_times()
        again = one_call(ctx, rs, prm, packs, qual_args)
        times_off = ctx.kernel_times()
    finally:
        ctx.set_verify_streams(False)
        ctx.lib.cl_ctx_set_timing(ctx.h, 0)
    assert on_one[:4] == off_one[:4], "one-call driver: parts differ with the check on"
    assert on_chunked[:4] == off_chunked[:4], "chunked compressor: parts differ with the check on"
    assert again[:4] == off_one[:4]
    d1, d2 = _delta(v0, v1), _delta(v1, v2)
    for d, out in ((d1, on_one), (d2, on_chunked)):
        assert d[0] == len(out[1]) + len(out[3]), "parts checked != dna parts + qual parts returned"
        assert d[2] == sum(out[1]) + sum(out[3]), "bytes checked != the sum of the returned part sizes"
    assert d1[0] > 0 and d1[1] > 0 and d1[1] == d2[1], "the two drivers checked different numbers of symbols"
    assert launches_on > 0, "k_range_check was not launched with the check on"
    assert ctx.verified_streams() == v2, "the check ran although it was switched off"
    assert "k_range_code" in times_off and "k_range_check" not in times_off, "k_range_check launched although the check was switched off"


def test_wide_dna_keys_verify_streams_in_a_process_of_its_own():
    """COLORD_HIP_DNA_WIDE_KEYS is read when a coder is made: the level-1 golden once more with 64-bit sort keys."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", "test_drivers_verify_streams_and_write_the_same_parts and s6m_ont"],
                       capture_output=True, text=True, env=dict(os.environ, COLORD_HIP_DNA_WIDE_KEYS="1"), cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def _streams(path):
    return {name: [(m, hashlib.sha256(p).hexdigest()) for m, p in s.parts] for name, s in AR.read_archive(path).items() if name != "info"}


@pytest.mark.skipif(not os.path.exists(CLI), reason="needs colord_amd/colord_hip")
@pytest.mark.parametrize("extra", [[], ["--stream-input"], ["-G", "GENOME", "-s"], ["--gpus", "2", "--gpu-list", "0,0", "--transport", "host"]], ids=["plain", "stream_input", "genome", "two_ranks"])
def test_cli_verify_streams_changes_no_byte(tmp_path, extra):
    fq, gen = str(tmp_path / "M.bovis.fastq"), str(tmp_path / "M.bovis-reference.fna")
    open(fq, "wb").write(gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis.fastq.gz"), "rb").read())
    if "-G" in extra:
        open(gen, "wb").write(gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis-reference.fna.gz"), "rb").read())
        extra = [gen if x == "GENOME" else x for x in extra]
    plain, checked = str(tmp_path / "off.colord"), str(tmp_path / "on.colord")
    subprocess.check_call([CLI, "compress-ont"] + extra + [fq, plain])
    r = subprocess.run([CLI, "compress-ont", "--verify-streams", "--verify-scripts", "-v"] + extra + [fq, checked], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert _streams(checked) == _streams(plain)
    lines = re.findall(r"# coded streams verified[^:]*: (\d+) parts, (\d+) symbols, (\d+) bytes decode to the models' intervals", r.stderr)
    ar = AR.read_archive(checked)
    coded = [p for name in ("dna", "qual") if name in ar for _, p in ar[name].parts]
    assert lines and len(lines) == (2 if "--gpus" in extra else 1), r.stderr
    assert sum(int(l[0]) for l in lines) == len(coded), r.stderr
    assert sum(int(l[2]) for l in lines) == sum(len(p) for p in coded), r.stderr
    assert "# edit scripts verified" in r.stderr
