"""CPU suite for the model domains of the quality stream (no GPU needed): the option of `colord_hip compress-*` and its refusals; an
archive with a `hipqdomains` stream — a fixture written on the GPU by tools/make_qdomains_fixture.py — decoded on the host as one chain
with fresh models at every domain; and the new host code (the `hipqdomains` parser and the batching of whole domains in
csrc/cli/reader.hpp) under AddressSanitizer and UBSan as a program of its own (tests/tools/qdomains_host_test.cpp)."""
import gzip
import os
import struct
import subprocess
import pytest
from colord_amd import archive as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
FIX = os.path.join(ROOT, "tests", "golden", "qdomains")
ARC, FQ = os.path.join(FIX, "qdomains.colord"), os.path.join(FIX, "reads.fastq.gz")
HIPCC = "/opt/rocm/bin/hipcc"


# ---- the option ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,why", [(["compress-ont", "--gpus", "2"], "--gpus"), (["compress-ont", "--domains", "2"], "--domains"), (["compress-ont", "-q", "none"], "-q none"),
                                      (["compress-pbraw"], "-q none")])
def test_refused_combinations(tmp_path, args, why):
    out = str(tmp_path / "no.colord")
    r = subprocess.run([CLI] + args + ["--qual-domain-symbols", "60000", "in.fastq", out], capture_output=True, text=True)
    assert r.returncode == 1 and "--qual-domain-symbols" in r.stderr and why in r.stderr, r.stderr
    assert not os.path.exists(out)


def test_option_parsing():
    r = subprocess.run([CLI, "compress-ont", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--qual-domain-symbols N" in r.stderr and "hipqdomains" in r.stderr and "CANNOT read" in r.stderr
    assert "decompress [--ignore-digest] [--gpu N]" in r.stderr and "check [--gpu N]" in r.stderr
    r = subprocess.run([CLI, "compress-ont", "--qual-domain-symbols", "0", "a", "b"], capture_output=True, text=True)
    assert r.returncode == 1 and "must be positive" in r.stderr
    r = subprocess.run([CLI, "compress-ont", "--qual-domain-symbols"], capture_output=True, text=True)
    assert r.returncode == 1 and "needs a value" in r.stderr
    # accepted with the options it works with: the command line is then only short of its paths
    r = subprocess.run([CLI, "compress-ont", "--qual-domain-symbols", "8388608", "--stream-input", "--part-symbols", "4096", "--digest", "--verify-scripts", "--verify-streams", "in.fq"], capture_output=True, text=True)
    assert r.returncode == 1 and "expected input and output paths" in r.stderr and "unknown option" not in r.stderr


# ---- the fixture decodes on the host ------------------------------------------------------------------------------------------------
def domains_of(path):
    b = AR.read_archive(path)["hipqdomains"].parts[0][1]
    n = struct.unpack_from("<Q", b)[0]
    return [struct.unpack_from("<QQ", b, 8 + 16 * i) for i in range(n)]


def test_fixture_has_domains():
    a = AR.read_archive(ARC)
    d = domains_of(ARC)
    assert len(d) >= 3 and d[0] == (0, 0) and len(a["hipqdomains"].parts[0][1]) == 8 + 16 * len(d)
    assert all(y[0] - x[0] >= 2 and y[1] > x[1] for x, y in zip(d, d[1:])) and d[-1][0] < len(a["qual"].parts)
    assert len(a["qual"].parts) == len(a["dna"].parts) and "hipdigest" in a and "hipdomains" not in a


def test_fixture_decodes_on_the_host_to_its_fastq(tmp_path):
    out = str(tmp_path / "o.fastq")
    r = subprocess.run([CLI, "decompress", ARC, out], capture_output=True, text=True)
    assert r.returncode == 0 and "content digest: ok (dna, qual, header)" in r.stderr, r.stderr
    assert open(out, "rb").read() == gzip.open(FQ, "rb").read()
    r = subprocess.run([CLI, "check", ARC], capture_output=True, text=True)
    assert r.returncode == 0 and "content digest: ok (dna, qual, header)" in r.stdout, r.stdout


def test_gpu_switch_leaves_other_archives_on_the_host(tmp_path):
    """an archive without `hipqdomains` under --gpu: the host path, with a line saying why; no device is initialised"""
    out = str(tmp_path / "o.fastq")
    arc = os.path.join(ROOT, "tests", "golden", "archives", "c1_ont_default.colord")
    r = subprocess.run([CLI, "decompress", "--gpu", "0", arc, out], capture_output=True, text=True)
    assert r.returncode == 0 and "no `hipqdomains` stream" in r.stderr and "decoded on the host" in r.stderr, r.stderr
    ref = str(tmp_path / "r.fastq")
    subprocess.check_call([CLI, "decompress", arc, ref], stderr=subprocess.DEVNULL)
    assert open(out, "rb").read() == open(ref, "rb").read()


# ---- the new host code under the sanitizers, as a program of its own ------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "qdomains_host_test")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "include"),
                           "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "tools", "qdomains_host_test.cpp"), "-o", exe, "-lz"])
    return exe


def test_parser_and_batching_under_sanitizers(sanitized_program):
    """part by part and in batches of whole domains (several batches): the same records, the FASTQ's, and the stored digests"""
    r = subprocess.run([sanitized_program, ARC, "50000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    nd = len(domains_of(ARC))
    fq = gzip.open(FQ, "rb").read().decode().split("\n")
    n = (len(fq) - 1) // 4
    tail = lines[-1].split()
    assert nd >= 3 and tail[0] == "ok:" and int(tail[1]) == n and int(tail[3]) == nd and int(tail[5]) >= 3 and int(tail[8]) == nd, lines[-1]   # several batches
    assert lines[3:3 + n] == [fq[4 * i + 1] + "\t" + fq[4 * i + 3] for i in range(n)]
    chk = subprocess.run([CLI, "check", ARC], capture_output=True, text=True).stdout.splitlines()
    assert lines[:3] == chk[:3]
    # one batch for everything, and a batch per domain
    for mb, want in (("1000000000", 1), ("1", nd)):
        r = subprocess.run([sanitized_program, ARC, mb], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and int(r.stdout.splitlines()[-1].split()[5]) == want, r.stdout[-500:] + r.stderr[-2000:]


def corrupt(tmp_path, name, payload):
    a = AR.read_archive(ARC)
    a["hipqdomains"].parts[0] = (0, payload)
    path = str(tmp_path / (name + ".colord"))
    AR.write_archive(path, list(a.values()))
    return path


def test_a_corrupt_domain_stream_is_an_exception_with_a_message(sanitized_program, tmp_path):
    good = AR.read_archive(ARC)["hipqdomains"].parts[0][1]
    n = struct.unpack_from("<Q", good)[0]
    n_parts = len(AR.read_archive(ARC)["qual"].parts)
    cases = {
        "truncated": good[:-5],
        "cut_to_its_count": good[:8],
        "empty": b"",
        "count_too_large": struct.pack("<Q", n + 1) + good[8:],
        "count_huge": struct.pack("<Q", 1 << 62) + good[8:],
        "count_zero": struct.pack("<Q", 0),
        "trailing_bytes": good + b"\0" * 16,
        "first_not_zero": good[:8] + struct.pack("<QQ", 1, 0) + good[24:],
        "descending": good[:24] + struct.pack("<QQ", 0, 0) + good[40:],
        "behind_the_parts": good[:-16] + struct.pack("<QQ", n_parts, struct.unpack_from("<Q", good, len(good) - 8)[0]),
        "reads_beyond_the_file": good[:-8] + struct.pack("<Q", 1 << 40),     # (found where the domain starts: the decoder counts the reads itself)
        "first_read_off_by_one": good[:32] + struct.pack("<Q", struct.unpack_from("<Q", good, 32)[0] + 1) + good[40:],
    }
    same = corrupt(tmp_path, "same", good)                                  # (the rewritten container itself is fine)
    assert subprocess.run([sanitized_program, same], capture_output=True, text=True, timeout=300).returncode == 0
    for name, payload in cases.items():
        path = corrupt(tmp_path, name, payload)
        r = subprocess.run([sanitized_program, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 3 and r.stdout.startswith("error: ") and ("hipqdomains" in r.stdout or "truncated stream" in r.stdout), (name, r.stdout[-500:], r.stderr[-2000:])
        out = str(tmp_path / "o.fastq")
        c = subprocess.run([CLI, "decompress", path, out], capture_output=True, text=True)
        assert c.returncode == 1 and "colord_hip:" in c.stderr and not os.path.exists(out), (name, c.stderr)


def test_a_wrong_but_well_formed_domain_stream_fails_the_digest(tmp_path):
    """a domain start moved by a part, with the read that part starts at: the models start afresh in the wrong place, what decodes is not
    what was compressed"""
    a = AR.read_archive(ARC)
    good = bytearray(a["hipqdomains"].parts[0][1])
    first_read = [0]
    for n_reads, _ in a["dna"].parts:
        first_read.append(first_read[-1] + n_reads)
    p1, r1 = struct.unpack_from("<QQ", good, 24)
    assert r1 == first_read[p1]
    struct.pack_into("<QQ", good, 24, p1 + 1, first_read[p1 + 1])
    path = corrupt(tmp_path, "moved", bytes(good))
    out = str(tmp_path / "o.fastq")
    r = subprocess.run([CLI, "decompress", path, out], capture_output=True, text=True)
    assert r.returncode == 1 and "content digest mismatch" in r.stderr and "qual" in r.stderr and not os.path.exists(out), r.stderr
