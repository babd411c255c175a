"""GPU suite for `colord_hip compress-* --qual-domain-symbols` and `colord_hip decompress / check --gpu`: the option touches the `qual`
stream alone, and an archive with `hipqdomains` decodes to the same file on the host (one chain, fresh models at every domain) and on
the device (one lane per domain)."""
import hashlib
import os
import subprocess
import numpy as np
import pytest
from colord_amd import archive as AR
from colord_amd.fastq import write_fastq
from colord_amd.synth import make_reads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
OPT = ["--part-symbols", "4096", "--digest"]
DOM = ["--qual-domain-symbols", "60000"]


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def run(args):
    r = subprocess.run([CLI] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """a FASTQ of about 2 Mbases, and its archives with -q org: without the option, with it, and with it under --stream-input"""
    d = tmp_path_factory.mktemp("qdom")
    rs = make_reads(seed=12, genome_len=100_000, target_bases=2_000_000, mean_scale=3000.0, n_frac=0.1)
    rng = np.random.default_rng(12)
    rs.quals = (33 + np.clip(rng.normal(22, 9, len(rs.quals)), 0, 60).astype(np.uint8)).astype(np.uint8)
    fq = str(d / "in.fastq")
    write_fastq(fq, rs)
    w = dict(dir=d, fq=fq, plain=str(d / "plain.colord"), dom=str(d / "dom.colord"))
    run(["compress-ont", "-q", "org"] + OPT + [fq, w["plain"]])
    run(["compress-ont", "-q", "org"] + OPT + DOM + [fq, w["dom"]])
    return w


def streams(path):
    return {n: [(m, hashlib.sha256(p).hexdigest()) for m, p in s.parts] for n, s in AR.read_archive(path).items()}


def both_ways(work, arc, tag):
    """decompress on the host and with --gpu 0 -> (host file, device file); both check forms print the same and exit 0"""
    host, dev = str(work["dir"] / (tag + ".host.fastq")), str(work["dir"] / (tag + ".gpu.fastq"))
    r = run(["decompress", arc, host])
    assert "content digest: ok (dna, qual, header)" in r.stderr and "decoded on GPU" not in r.stderr
    r = run(["decompress", "--gpu", "0", arc, dev])
    assert "content digest: ok (dna, qual, header)" in r.stderr and "quality stream decoded on GPU 0" in r.stderr
    a, b = run(["check", arc]), run(["check", "--gpu", "0", arc])
    assert a.stdout == b.stdout and "content digest: ok" in a.stdout
    return host, dev


def test_the_option_touches_the_qual_stream_alone(work):
    a, b = streams(work["plain"]), streams(work["dom"])
    assert set(b) == set(a) | {"hipqdomains"}
    for name in ("dna", "header", "hipdigest", "meta"):
        assert a[name] == b[name], name
    assert a["qual"] != b["qual"] and len(a["qual"]) == len(b["qual"])
    q = AR.read_archive(work["dom"])["hipqdomains"].parts[0][1]
    v = np.frombuffer(q, "<u8")
    n = int(v[0])
    assert n >= 20 and len(v) == 1 + 2 * n and v[1] == 0 and v[2] == 0
    assert np.all(np.diff(v[1::2].astype(np.int64)) >= 2)                       # first parts: domains of several parts
    # the first domain is coded as without the option
    first = int(v[3])
    assert a["qual"][:first] == b["qual"][:first] and a["qual"][first] != b["qual"][first]


def test_host_and_device_decode_to_the_input(work):
    host, dev = both_ways(work, work["dom"], "org")
    assert sha(host) == sha(dev) == sha(work["fq"])


def test_several_batches_on_the_device_give_the_same_file_and_digest(work):
    """COLORD_HIP_QDEC_BATCH_BASES small: the quality thread hands the domains to the device in many batches — each starts at a domain, its
    reads are digested at their index in the whole input, and the qualities go on in file order"""
    out = str(work["dir"] / "batches.fastq")
    for bases in ("150000",):
        r = subprocess.run([CLI, "decompress", "--gpu", "0", work["dom"], out], capture_output=True, text=True, env=dict(os.environ, COLORD_HIP_QDEC_BATCH_BASES=bases))
        assert r.returncode == 0 and "content digest: ok (dna, qual, header)" in r.stderr, r.stderr[-2000:]
        line = [l for l in r.stderr.splitlines() if "quality stream decoded on GPU 0" in l][0].split()
        n_dom, n_batch = int(line[line.index("model") - 1]), int(line[line.index("batch(es),") - 1])
        assert n_dom >= 20 and 5 <= n_batch < n_dom, line
        assert sha(out) == sha(work["fq"])
    r = subprocess.run([CLI, "check", "--gpu", "0", work["dom"]], capture_output=True, text=True, env=dict(os.environ, COLORD_HIP_QDEC_BATCH_BASES="150000"))
    assert r.returncode == 0 and r.stdout == run(["check", work["dom"]]).stdout


def test_gpu_number_is_parsed_strictly(work):
    r = subprocess.run([CLI, "decompress", "--gpu", "x", work["dom"], str(work["dir"] / "x.fastq")], capture_output=True, text=True)
    assert r.returncode == 1 and "--gpu needs a device number" in r.stderr and not os.path.exists(str(work["dir"] / "x.fastq"))


def test_lossy_mode_decodes_the_same_on_both_paths(work):
    arc = str(work["dir"] / "avg4.colord")
    run(["compress-ont", "-q", "4-avg"] + OPT + DOM + [work["fq"], arc])
    host, dev = both_ways(work, arc, "avg4")
    assert sha(host) == sha(dev) != sha(work["fq"])
    plain = str(work["dir"] / "avg4.plain.colord")
    run(["compress-ont", "-q", "4-avg"] + OPT + [work["fq"], plain])
    assert streams(plain)["hipdigest"] == streams(arc)["hipdigest"]


def test_stream_input_writes_the_same_archive(work):
    arc = str(work["dir"] / "si.colord")
    run(["compress-ont", "-q", "org", "--stream-input", "--chunk-bases", "5e5", "--verify-streams", "--verify-scripts"] + OPT + DOM + [work["fq"], arc])
    a = streams(arc)
    ref = str(work["dir"] / "si.ref.colord")
    run(["compress-ont", "-q", "org", "--chunk-bases", "5e5"] + OPT + DOM + [work["fq"], ref])
    b = streams(ref)
    for name in b:
        if name != "info":
            assert a[name] == b[name], name
    host, dev = both_ways(work, arc, "si")
    assert sha(host) == sha(dev) == sha(work["fq"])


def test_an_archive_without_domains_takes_the_host_path_under_gpu(work):
    out = str(work["dir"] / "plain.fastq")
    r = run(["decompress", "--gpu", "0", work["plain"], out])
    assert "no `hipqdomains` stream" in r.stderr and "decoded on GPU" not in r.stderr
    assert sha(out) == sha(work["fq"])


@pytest.mark.parametrize("extra,why", [(["--gpus", "2"], "--gpus"), (["--domains", "2"], "--domains"), (["-q", "none"], "-q none")])
def test_refused_combinations(work, extra, why):
    r = subprocess.run([CLI, "compress-ont"] + DOM + extra + [work["fq"], str(work["dir"] / "no.colord")], capture_output=True, text=True)
    assert r.returncode == 1 and "--qual-domain-symbols" in r.stderr and why in r.stderr
    assert not os.path.exists(str(work["dir"] / "no.colord"))
