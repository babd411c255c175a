"""CPU suite of the qual-values digest (kind 4; `colord_hip compress-* --digest-values`, `decompress`, `check`).  The judge is
tests/qual_values_ref.py — the decoder's double recurrence and the integer formula, both derived from the INPUT qualities — first checked
against itself, then: the host functions of the C ABI on the input reads of the nine reference-written archives with a coded quality
stream == the quality lines `colord_hip decompress` returns for them (pinned by SHA-256 to the reference's decompressor) == the
reference; archives stamped with a version-2 `hipdigest` stream; the host loops of csrc/digest.hpp under AddressSanitizer and UBSan as a
program of its own.  No GPU is needed."""
import ctypes as C
import gzip
import hashlib
import json
import os
import re
import struct
import subprocess
import numpy as np
import pytest
from colord_amd import _native as N, archive as AR
import digest_ref as R
import qual_values_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARC = os.path.join(ROOT, "tests", "golden", "archives")
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
EXP = json.load(open(os.path.join(ARC, "expected.json")))
# the nine golden archives with a coded quality stream (first 24 reads of tests/data/M.bovis.fastq.gz, default -T / -D): name -> mode
CODED = {"bovis24_q_org_balanced": "org", "bovis24_org_ratio": "org", "bovis24_q_2-fix_balanced": "2-fix", "bovis24_q_4-fix_balanced": "4-fix", "bovis24_q_5-fix_balanced": "5-fix",
         "bovis24_q_2-avg_balanced": "2-avg", "bovis24_q_4-avg_balanced": "4-avg", "bovis24_q_5-avg_balanced": "5-avg", "bovis24_q_avg_balanced": "avg"}
ALL_MODES = ["org", "5-avg", "4-avg", "2-avg", "5-fix", "4-fix", "2-fix", "avg"]


def qual_params(mode, T=None, D=None):
    fwd = list(R.DEFAULT_T.get(mode, ()) if T is None else T)
    rev = list(R.DEFAULT_D.get(mode, ()) if D is None else D)
    p = N.QualParams(mode=R.QUAL_MODES.index(mode), source=0, level=1, n_fwd=len(fwd), n_rev=len(rev))
    for i, v in enumerate(fwd):
        p.fwd[i] = v
    for i, v in enumerate(rev):
        p.rev[i] = v
    return p


def host_values(mode, reads_ascii, T=None, D=None):
    """cl_qual_values_host: per read the ASCII bytes the decoder will write, from its input quality bytes"""
    lib = N.load()
    q = np.ascontiguousarray(np.concatenate(reads_ascii) if reads_ascii else np.zeros(0, np.uint8), dtype=np.uint8)
    off = np.cumsum([0] + [len(r) for r in reads_ascii]).astype(np.uint64)
    out = np.full(len(q) + 16, 0xEE, np.uint8)
    prm = qual_params(mode, T, D)
    assert lib.cl_qual_values_host(C.byref(prm), q.ctypes.data, off.ctypes.data, len(reads_ascii), out.ctypes.data) == 0
    assert (out[len(q):] == 0xEE).all()
    return [out[off[i]:off[i + 1]].copy() for i in range(len(reads_ascii))]


def host_digest(reads_ascii, first_read=0, acc=None):
    """cl_digest_qual_values_host over decoded quality lines"""
    lib = N.load()
    q = np.ascontiguousarray(np.concatenate(reads_ascii) if reads_ascii else np.zeros(0, np.uint8), dtype=np.uint8)
    off = np.cumsum([0] + [len(r) for r in reads_ascii]).astype(np.uint64)
    acc = N.Digest() if acc is None else acc
    assert lib.cl_digest_qual_values_host(q.ctypes.data, off.ctypes.data, len(reads_ascii), first_read, C.byref(acc)) == 0
    return acc.triple()


def hand_made_reads(seed=1):
    """input quality reads (ASCII) where the loops can go wrong: empty, 1 / 7 / 8 / 9, one bin only, bins alternating, 0 and 95, random"""
    rng = np.random.default_rng(seed)
    wide = np.array([0, 3, 6, 7, 10, 13, 14, 20, 25, 26, 40, 92, 93, 95], np.uint8)
    reads = [rng.choice(wide, L) for L in (0, 1, 7, 8, 9, 63, 64, 65, 513)]
    reads.append(np.full(100, 30, np.uint8))                                  # one bin
    reads.append(np.tile(np.array([2, 40], np.uint8), 60))                    # alternating
    reads.append(np.array([0, 95, 0, 95, 95], np.uint8))
    reads += [rng.integers(0, 94, int(L)).astype(np.uint8) for L in rng.integers(1, 400, 8)]
    return [(r + 33).astype(np.uint8) for r in reads]


# ---- the reference against itself -----------------------------------------------------------------------------------------------------
def test_reference_double_recurrence_equals_integer_formula():
    rng = np.random.default_rng(7)
    for mode in ALL_MODES:
        for T in (None, [5, 5, 30] if mode[0] == "4" else None):
            for _ in range(6):
                p = rng.integers(0, 96, int(rng.integers(0, 700)))
                assert np.array_equal(V.values_double(mode, p, T), V.values_int(mode, p, T)), mode
    p = rng.integers(90, 96, 300_000)                                         # one bin, k A far beyond 2^32
    assert np.array_equal(V.values_double("avg", p), V.values_int("avg", p))
    assert np.array_equal(V.values_double("2-avg", p), V.values_int("2-avg", p))
    v = V.values_int("avg", p)
    assert abs(int(v.astype(np.int64).sum()) - int(p.sum())) <= 300_000 // 256 + 1      # the diffusion keeps the read's sum, to the average's truncation


def test_reference_values_of_simple_reads():
    assert V.values_int("org", [0, 95, 40]).tolist() == [0, 95, 40]
    assert V.values_int("2-fix", [0, 6, 7, 95]).tolist() == [1, 1, 13, 13]
    assert V.values_int("2-fix", [0, 6, 7, 95], T=[7], D=[5, 20]).tolist() == [5, 5, 20, 20]
    assert V.values_int("avg", [10, 11]).tolist() == [10, 11]                  # A = 10.5 * 256: floor(10.5), floor(21) - 10
    assert V.values_int("org", [-1, 96, 200]).tolist() == [0, 0, 0]            # outside Phred 0..95: 0


def test_reference_simple_two_bins():
    # bin 0 holds 1, 2, 2 (A = int(5 / 3 * 256) = 426): floor(426 k / 256) = 1, 3, 4 -> 1, 2, 1; bin 1 holds 20, 21 (A = 5248): 20, 41 -> 20, 21
    assert V.values_int("2-avg", [1, 20, 2, 21, 2]).tolist() == [1, 20, 2, 21, 1]


# ---- the host functions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ALL_MODES)
def test_host_values_equal_the_reference(mode):
    reads = hand_made_reads()
    cases = [(None, None)]
    if mode[0] in "245":
        n = int(mode[0])
        cases.append(([5] * 2 + list(range(30, 30 + n - 3)) if n > 2 else [0], list(range(40, 40 + n)) if mode.endswith("fix") else None))      # an empty bin; custom -D
        cases.append((list(range(10, 10 + n - 2)) + [96], [0, 222, 7, 9, 11][:n] if mode.endswith("fix") else None))                              # -T ending at 96; -D at its limits
    for T, D in cases:
        got = host_values(mode, reads, T, D)
        want = [V.values_int(mode, r.astype(np.int64) - 33, T, D) for r in reads]
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, (w.astype(np.int64) + 33).astype(np.uint8)), (mode, T, D, i, len(w))
        for first in (0, 5, 1 << 40):
            assert host_digest(got, first) == V.digest_values(want, first)
        cut = 7
        acc = N.Digest()
        host_digest(got[cut:], 3 + cut, acc)
        assert host_digest(got[:cut], 3, acc) == V.digest_values(want, 3)


def test_host_refuses_what_it_cannot_digest():
    lib = N.load()
    off = np.zeros(2, np.uint64); acc = N.Digest(); out = np.zeros(1, np.uint8)
    p = qual_params("2-fix", D=[1])                                            # *-fix without a -D value for every bin
    assert lib.cl_qual_values_host(C.byref(p), None, off.ctypes.data, 1, out.ctypes.data) == N.CL_E_INVALID
    p = qual_params("2-fix", D=[1, 223])
    assert lib.cl_qual_values_host(C.byref(p), None, off.ctypes.data, 1, out.ctypes.data) == N.CL_E_INVALID
    p = qual_params("4-avg", T=[7, 14])                                        # thresholds that do not fit the mode
    assert lib.cl_qual_values_host(C.byref(p), None, off.ctypes.data, 1, out.ctypes.data) == N.CL_E_INVALID
    p = qual_params("none")
    assert lib.cl_qual_values_host(C.byref(p), None, off.ctypes.data, 1, out.ctypes.data) == N.CL_E_INVALID
    assert lib.cl_digest_qual_values_host(None, off.ctypes.data, 1, (1 << 63) - 1, C.byref(acc)) == 0
    assert lib.cl_digest_qual_values_host(None, off.ctypes.data, 1, 1 << 63, C.byref(acc)) == N.CL_E_INVALID
    # kind 4 has functions of its own: the byte digest takes the kinds it took
    assert lib.cl_digest_bytes_host(4, None, off.ctypes.data, 1, 0, C.byref(acc)) == N.CL_E_INVALID


def test_binding_declares_the_new_entry_points():
    lib = N.load()
    for name in ("cl_digest_qual_values", "cl_qual_values", "cl_qual_values_host", "cl_digest_qual_values_host", "cl_ctx_set_digest_values", "cl_ctx_digest_values",
                 "cl_compressor_digest_values"):
        assert name in N.exported_names() and hasattr(lib, name)
    from colord_amd import device as D
    for name in ("qual_values", "digest_qual_values", "set_digest_values", "digest_values"):
        assert hasattr(D.Context, name)
    assert hasattr(D.Compressor, "digest_values")


# ---- the golden archives -----------------------------------------------------------------------------------------------------------------
def input_reads(n=24):
    """the quality lines (ASCII) of the first n reads of tests/data/M.bovis.fastq.gz: what the reference compressed"""
    lines = gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis.fastq.gz"), "rb").read().split(b"\n")
    return [np.frombuffer(lines[4 * i + 3], np.uint8) for i in range(n)]


@pytest.fixture(scope="module")
def decoded(tmp_path_factory):
    """name -> the quality lines of the FASTQ `colord_hip decompress` writes for a golden archive (its SHA-256 is the pinned one)"""
    cache = {}

    def get(name):
        if name not in cache:
            out = str(tmp_path_factory.mktemp("qv") / "out.fastq")
            r = subprocess.run([CLI, "decompress", os.path.join(ARC, name + ".colord"), out], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert hashlib.sha256(open(out, "rb").read()).hexdigest() == EXP[name]["decompressed_sha256"]
            cache[name] = R.parse_fastq(out)
        return cache[name]
    return get


def test_the_coded_set_is_the_nine_archives():
    assert len(CODED) == 9
    for name, mode in CODED.items():                                          # QualityComprMode: the byte of `meta` behind reference reads, candidates, level, source and size
        assert AR.read_archive(os.path.join(ARC, name + ".colord"))["meta"].parts[0][1][21] == R.QUAL_MODES.index(mode), name


@pytest.mark.parametrize("name", sorted(CODED))
def test_values_from_the_input_are_what_the_reference_archive_decodes_to(name, decoded):
    mode = CODED[name]
    src = input_reads()
    lines = [(r[2] + 33).astype(np.uint8) for r in decoded(name)]
    assert len(lines) == 24
    got = host_values(mode, src)
    want = [V.values_int(mode, r.astype(np.int64) - 33) for r in src]
    for i in range(24):
        assert np.array_equal(got[i], lines[i]), (name, i)                    # the library from the input == the reference's decoder
        assert np.array_equal(want[i].astype(np.int64) + 33, lines[i]), (name, i)      # the Python reference == the same
    assert host_digest(lines) == V.digest_values(want) == V.digest_values([r[2].astype(np.uint8) for r in decoded(name)])


# ---- archives stamped with a version-2 `hipdigest` stream ------------------------------------------------------------------------------
TRIPLE4 = re.compile(r"^(stored )?(dna|qual|header|qual-values) reads=(\d+) symbols=(\d+) sum=0x([0-9a-f]{16})$", re.M)


def parse_check4(text):
    return {("stored " if st else "") + name: (int(r), int(s), int(x, 16)) for st, name, r, s, x in TRIPLE4.findall(text)}


def triples_of(name, recs, D=None):
    """(dna, qual, header, qual-values) of a golden archive: dna and header from the decoded records, qual as `colord_hip check` computes it
    (its own tests pin it), qual-values from the INPUT by the Python reference"""
    mode = CODED[name]
    dna = R.digest_bases([r[1] for r in recs])
    header = R.digest_bytes(R.HEADER, [R.header_bytes(r[0], r[3]) for r in recs])
    c = subprocess.run([CLI, "check", os.path.join(ARC, name + ".colord")], capture_output=True, text=True)
    assert c.returncode == 0
    qual = parse_check4(c.stdout)["qual"]
    qval = V.digest_input(mode, [r.astype(np.int64) - 33 for r in input_reads()], 0, None, D)
    return dna, qual, header, qval


def stamp(name, path, payload):
    arc = AR.read_archive(os.path.join(ARC, name + ".colord"))
    AR.write_archive(path, list(arc.values()) + [AR.Stream("hipdigest", 0, [(0, payload)])])


STAMPED = ["bovis24_q_4-avg_balanced", "bovis24_q_5-fix_balanced"]


@pytest.mark.parametrize("name", STAMPED)
def test_version_2_stream_checks_four_digests(name, decoded, tmp_path):
    arc, out = str(tmp_path / "s.colord"), str(tmp_path / "o.fastq")
    t = triples_of(name, decoded(name))
    payload = V.pack_hipdigest2(*t)
    assert len(payload) == 104
    stamp(name, arc, payload)
    r = subprocess.run([CLI, "decompress", arc, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "content digest: ok (dna, qual, qual-values, header)" in r.stderr
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == EXP[name]["decompressed_sha256"]
    c = subprocess.run([CLI, "check", arc], capture_output=True, text=True)
    assert c.returncode == 0 and "content digest: ok (dna, qual, qual-values, header)" in c.stdout, c.stdout
    got = parse_check4(c.stdout)
    for k, want in zip(("dna", "qual", "header", "qual-values"), t):
        assert got[k] == want == got["stored " + k], k
    i = subprocess.run([CLI, "info", arc], capture_output=True, text=True)
    assert i.returncode == 0 and "content digest: qual-values reads=24 symbols=%d sum=0x%016x" % (t[3][1], t[3][2]) in i.stderr
    assert i.stderr.count("content digest: ") == 4


@pytest.mark.parametrize("name,how", [(STAMPED[0], "flip"), (STAMPED[1], "flip"), (STAMPED[1], "other_D")])
def test_wrong_qual_values_are_refused_and_only_they_are_named(name, how, decoded, tmp_path):
    arc, out = str(tmp_path / "s.colord"), str(tmp_path / "o.fastq")
    dna, qual, header, qval = triples_of(name, decoded(name))
    bad = (qval[0], qval[1], qval[2] ^ (1 << 9)) if how == "flip" else triples_of(name, decoded(name), D=[3, 10, 18, 36, 93])[3]
    assert bad != qval and bad[:2] == qval[:2]
    stamp(name, arc, V.pack_hipdigest2(dna, qual, header, bad))
    r = subprocess.run([CLI, "decompress", arc, out], capture_output=True, text=True)
    assert r.returncode == 1, r.stderr
    assert "content digest mismatch" in r.stderr and "stored qual-values reads=" in r.stderr and "computed qual-values reads=" in r.stderr
    for other in ("dna", "qual", "header"):
        assert f"stored {other} " not in r.stderr
    assert not os.path.exists(out)
    c = subprocess.run([CLI, "check", arc], capture_output=True, text=True)
    assert c.returncode == 1 and "content digest mismatch: stored qual-values" in c.stdout and "stored dna reads" in c.stdout       # (the stored lines are listed, the mismatch names one)
    assert c.stdout.split("content digest mismatch:")[1].count("stored ") == 1
    r = subprocess.run([CLI, "decompress", "--ignore-digest", arc, out], capture_output=True, text=True)
    assert r.returncode == 0 and "content digest" not in r.stderr
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == EXP[name]["decompressed_sha256"]


def test_version_1_stream_still_checks_three(decoded, tmp_path):
    name = STAMPED[0]
    arc, out = str(tmp_path / "s.colord"), str(tmp_path / "o.fastq")
    dna, qual, header, qval = triples_of(name, decoded(name))
    stamp(name, arc, R.pack_hipdigest(dna, qual, header))
    r = subprocess.run([CLI, "decompress", arc, out], capture_output=True, text=True)
    assert r.returncode == 0 and "content digest: ok (dna, qual, header)" in r.stderr, r.stderr
    c = subprocess.run([CLI, "check", arc], capture_output=True, text=True)
    assert c.returncode == 0 and "content digest: ok (dna, qual, header)" in c.stdout
    got = parse_check4(c.stdout)
    assert got["qual-values"] == qval and "stored qual-values" not in got      # `check` computes the fourth for any coded quality stream


@pytest.mark.parametrize("name", sorted(CODED))
def test_check_prints_the_computed_qual_values_of_a_reference_archive(name):
    c = subprocess.run([CLI, "check", os.path.join(ARC, name + ".colord")], capture_output=True, text=True)
    assert c.returncode == 0, c.stdout + c.stderr
    assert parse_check4(c.stdout)["qual-values"] == V.digest_input(CODED[name], [r.astype(np.int64) - 33 for r in input_reads()])


def test_check_prints_no_qual_values_without_a_coded_quality_stream():
    c = subprocess.run([CLI, "check", os.path.join(ARC, "bovis24_q_none_balanced.colord")], capture_output=True, text=True)
    assert c.returncode == 0 and "qual-values" not in c.stdout


@pytest.mark.parametrize("how", ["version_3", "100_bytes", "version_1_of_104", "version_2_of_80"])
def test_a_stream_of_another_shape_cannot_be_read(how, decoded, tmp_path):
    name = STAMPED[0]
    arc, out = str(tmp_path / "s.colord"), str(tmp_path / "o.fastq")
    good = V.pack_hipdigest2(*triples_of(name, decoded(name)))
    payload = {"version_3": struct.pack("<I", 3) + good[4:], "100_bytes": good[:100], "version_1_of_104": struct.pack("<I", 1) + good[4:],
               "version_2_of_80": good[:80]}[how]
    stamp(name, arc, payload)
    r = subprocess.run([CLI, "decompress", arc, out], capture_output=True, text=True)
    assert r.returncode == 1 and "is not one this build reads" in r.stderr and not os.path.exists(out)
    c = subprocess.run([CLI, "check", arc], capture_output=True, text=True)
    assert c.returncode == 1 and "is not one this build reads" in c.stdout


def test_help_names_the_option():
    r = subprocess.run([CLI, "compress-ont", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--digest-values" in r.stderr and "qual-values" in r.stderr
    r = subprocess.run([CLI, "compress-ont", "--digest-values", "in.fq"], capture_output=True, text=True)
    assert r.returncode == 1 and "expected input and output paths" in r.stderr and "unknown option" not in r.stderr


# ---- the host loops under AddressSanitizer and UBSan, as a program of its own ------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    """tests/tools/qual_values_host_test.cpp: csrc/digest.hpp under a host compiler alone (it needs no HIP), the sanitizers' runtimes linked in;
    it has its own main and runs as it is, nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("san") / "qual_values_host_test")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "tools", "qual_values_host_test.cpp"), "-o", exe])
    return exe


def test_host_loops_under_sanitizers_equal_the_reference(sanitized_program, tmp_path):
    reads = hand_made_reads(seed=4)
    cases = [(m, None, None, 0, reads) for m in ALL_MODES]
    cases += [("4-avg", [5, 5, 30], None, 1 << 40, reads),                    # an empty bin
              ("5-fix", [3, 9, 9, 96], [0, 222, 7, 9, 11], 5, reads), ("avg", None, None, 3, []), ("2-avg", None, None, 3, [np.zeros(0, np.uint8)]),
              ("org", None, None, 0, [np.array([0, 32, 33, 128, 129, 255], np.uint8)])]      # bytes outside Phred+33 0..95
    blob = struct.pack("<Q", len(cases))
    for mode, T, D, first, rd in cases:
        p = qual_params(mode, T, D)
        off = np.cumsum([0] + [len(r) for r in rd]).astype("<u8")
        blob += struct.pack("<iI8II8IQQ", p.mode, p.n_fwd, *p.fwd, p.n_rev, *p.rev, first, len(rd)) + off.tobytes() + b"".join(r.tobytes() for r in rd)
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    r = subprocess.run([sanitized_program, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"ok: {len(cases)} cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = re.findall(r"^case reads=(\d+) symbols=(\d+) sum=0x([0-9a-f]{16}) values=([0-9a-f]*)$", r.stdout, re.M)
    assert len(got) == len(cases)
    for (mode, T, D, first, rd), (a, b, c, hexv) in zip(cases, got):
        want = [V.values_int(mode, x.astype(np.int64) - 33, T, D) for x in rd]
        assert (int(a), int(b), int(c, 16)) == V.digest_values(want, first), (mode, T)
        flat = np.concatenate(want).astype(np.int64) + 33 if want else np.zeros(0, np.int64)
        assert bytes.fromhex(hexv) == flat.astype(np.uint8).tobytes(), (mode, T)
