"""CPU suite of the content digest (`colord_hip compress-* --digest`, `decompress`, `check`): the host functions of the C ABI
and the digesting decoders against tests/digest_ref.py (numpy, written from the definition), on the reference-written archives of
tests/golden/archives — whose decompressed FASTQ is pinned by expected.json — and on archives stamped with a `hipdigest` stream here.
No GPU is needed: everything on this side of the archive is host code."""
import ctypes as C
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARC = os.path.join(ROOT, "tests", "golden", "archives")
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
EXP = json.load(open(os.path.join(ARC, "expected.json")))
GENOME = os.path.join(ROOT, "tests", "data", "M.bovis-reference.fna.gz")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
READ_LENS = (1, 2, 31, 32, 33, 63, 64, 65, 257)
BYTE_LENS = (1, 7, 8, 9, 4097)


def genome_args(name):
    return ["-G", GENOME] if name.endswith("_external") else []


def host_bases(reads, first_read=0, acc=None):
    lib = N.load()
    codes = np.ascontiguousarray(np.concatenate(reads) if reads else np.zeros(0, np.uint8), dtype=np.uint8)
    off = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    acc = N.Digest() if acc is None else acc
    assert lib.cl_digest_bases_host(codes.ctypes.data, off.ctypes.data, len(reads), first_read, C.byref(acc)) == 0
    return acc.triple()


def host_bytes(kind, seqs, first_read=0, acc=None):
    lib = N.load()
    b = np.ascontiguousarray(np.concatenate([np.frombuffer(bytes(s), np.uint8) for s in seqs]) if seqs else np.zeros(0, np.uint8), dtype=np.uint8)
    off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    acc = N.Digest() if acc is None else acc
    assert lib.cl_digest_bytes_host(kind, b.ctypes.data, off.ctypes.data, len(seqs), first_read, C.byref(acc)) == 0
    return acc.triple()


def case_reads():
    """Reads of the lengths at which a 32-base block begins, ends or is alone; N at positions 0, 31, 32 and last."""
    rng = np.random.default_rng(11)
    reads = [rng.integers(0, 4, L).astype(np.uint8) for L in READ_LENS]
    for L in (33, 64, 65, 257):
        for pos in (0, 31, 32, L - 1):
            r = rng.integers(0, 4, L).astype(np.uint8); r[pos] = 4
            reads.append(r)
    reads.append(np.array([4], np.uint8)); reads.append(np.full(32, 4, np.uint8))
    return reads


def case_bytes():
    rng = np.random.default_rng(12)
    return [rng.integers(0, 256, L).astype(np.uint8).tobytes() for L in BYTE_LENS]


# ---- host functions against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_read", [0, 7, 1 << 33])
def test_host_bases_equal_the_reference(first_read):
    reads = case_reads()
    assert host_bases(reads, first_read) == R.digest_bases(reads, first_read)
    for i, r in enumerate(reads):                                             # and read by read: a wrong term cannot hide behind another
        assert host_bases([r], first_read + i) == R.digest_bases([r], first_read + i), (i, len(r))


@pytest.mark.parametrize("kind", [R.QUAL, R.HEADER])
def test_host_bytes_equal_the_reference(kind):
    seqs = case_bytes()
    assert host_bytes(kind, seqs, 3) == R.digest_bytes(kind, seqs, 3)
    for i, s in enumerate(seqs):
        assert host_bytes(kind, [s], i) == R.digest_bytes(kind, [s], i), len(s)
    assert host_bytes(R.QUAL, seqs)[2] != host_bytes(R.HEADER, seqs)[2]      # the kind is part of the digest


def test_digests_of_disjoint_reads_add():
    reads, seqs = case_reads(), case_bytes()
    whole_b, whole_s = host_bases(reads, 5), host_bytes(R.HEADER, seqs, 5)
    for cut in range(len(reads) + 1):
        acc = N.Digest()
        host_bases(reads[cut:], 5 + cut, acc)                                 # (in either order)
        assert host_bases(reads[:cut], 5, acc) == whole_b
    for cut in range(len(seqs) + 1):
        acc = N.Digest()
        host_bytes(R.HEADER, seqs[:cut], 5, acc)
        assert host_bytes(R.HEADER, seqs[cut:], 5 + cut, acc) == whole_s


def test_digest_depends_on_content_place_and_order():
    reads, seqs = case_reads(), case_bytes()
    base = host_bases(reads, 0)
    assert host_bases(reads, 1)[2] != base[2]                                 # first_read + 1
    sw = list(reads); sw[3], sw[4] = sw[4], sw[3]
    assert host_bases(sw, 0)[:2] == base[:2] and host_bases(sw, 0)[2] != base[2]      # two reads swapped: same counts, other sum
    for ri, pos in ((8, 0), (8, 256), (5, 31), (6, 32)):                      # one base changed
        ch = [r.copy() for r in reads]; ch[ri][pos] = (ch[ri][pos] + 1) & 3
        assert host_bases(ch, 0)[2] != base[2]
    a = [np.array([0, 1, 2, 0], np.uint8)]; n = [np.array([0, 1, 2, 4], np.uint8)]
    assert host_bases(a)[2] != host_bases(n)[2] and host_bases(a)[2] == R.digest_bases(a)[2]      # N <-> A
    sb = host_bytes(R.QUAL, seqs, 0)
    ch = list(seqs); ch[4] = ch[4][:4000] + bytes([ch[4][4000] ^ 1]) + ch[4][4001:]
    assert host_bytes(R.QUAL, ch, 0)[2] != sb[2]                              # one symbol
    one, padded = [b"\x05\x06\x07"], [b"\x05\x06\x07\x00"]                    # a zero byte appended: the words are the same, n is not
    assert np.array_equal(R.byte_words(one[0]), R.byte_words(padded[0]))
    assert host_bytes(R.QUAL, one)[2] != host_bytes(R.QUAL, padded)[2]
    assert host_bytes(R.QUAL, padded) == R.digest_bytes(R.QUAL, padded)


def test_read_indices_stay_below_2_63():
    lib = N.load()
    off = np.zeros(2, np.uint64); acc = N.Digest()
    assert lib.cl_digest_bases_host(None, off.ctypes.data, 1, (1 << 63) - 1, C.byref(acc)) == 0
    assert lib.cl_digest_bases_host(None, off.ctypes.data, 1, 1 << 63, C.byref(acc)) == N.CL_E_INVALID
    assert lib.cl_digest_bytes_host(R.HEADER, None, off.ctypes.data, 1, (1 << 64) - 1, C.byref(acc)) == N.CL_E_INVALID
    assert lib.cl_digest_bytes_host(7, None, off.ctypes.data, 1, 0, C.byref(acc)) == N.CL_E_INVALID


def test_binding_declares_the_new_entry_points():
    lib = N.load()
    for name in ("cl_ctx_set_digest", "cl_ctx_digest", "cl_compressor_digest", "cl_digest_bases", "cl_digest_quals", "cl_digest_bases_host", "cl_digest_bytes_host",
                 "cl_qual_decoder_set_digest", "cl_qual_decoder_digest"):
        assert name in N.exported_names() and hasattr(lib, name)
    from colord_amd import device as D
    for name in ("set_digest", "digest", "digest_bases", "digest_quals"):
        assert hasattr(D.Context, name)
    assert hasattr(D.Compressor, "digest")


# ---- the golden archives -----------------------------------------------------------------------------------------------------------
TRIPLE = re.compile(r"^(stored )?(dna|qual|header) reads=(\d+) symbols=(\d+) sum=0x([0-9a-f]{16})$", re.M)


def parse_check(text):
    out = {}
    for stored, name, r, s, x in TRIPLE.findall(text):
        out[("stored " if stored else "") + name] = (int(r), int(s), int(x, 16))
    return out


def run_check(path, name=""):
    return subprocess.run([CLI, "check"] + genome_args(name) + [path], capture_output=True, text=True, timeout=300)


def qual_mode_of(arc):
    """QualityComprMode of a FASTQ archive: the byte of `meta` behind reference reads, candidates, level, source and size."""
    return arc["meta"].parts[0][1][21] if "qual" in arc else None


@pytest.fixture(scope="module")
def decoded(tmp_path_factory):
    """name -> the records of the FASTQ `colord_hip decompress` writes (its SHA-256 is the pinned one), once for the module."""
    cache = {}

    def get(name):
        if name not in cache:
            out = str(tmp_path_factory.mktemp("dec") / "out.fastq")
            r = subprocess.run([CLI, "decompress"] + genome_args(name) + [os.path.join(ARC, name + ".colord"), out], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert hashlib.sha256(open(out, "rb").read()).hexdigest() == EXP[name]["decompressed_sha256"]
            assert "content digest" not in r.stderr                           # an archive without the stream: no digest line
            cache[name] = R.parse_fastq(out)
        return cache[name]
    return get


def reference_triples(name, recs):
    """(dna, header, qual or None) of the decoded records from the definition; qual where the symbols follow from the quality values."""
    arc = AR.read_archive(os.path.join(ARC, name + ".colord"))
    mode = qual_mode_of(arc)
    dna = R.digest_bases([r[1] for r in recs])
    header = R.digest_bytes(R.HEADER, [R.header_bytes(r[0], r[3]) for r in recs])
    qual = None
    if mode == 0:
        qual = R.digest_bytes(R.QUAL, [r[2].astype(np.uint8) for r in recs])
    elif mode in (4, 5, 6):                                                   # *-fix: the decoder wrote the -D value of the bin; the values are distinct
        vals = R.DEFAULT_D[R.QUAL_MODES[mode]]
        qual = R.digest_bytes(R.QUAL, [np.array([vals.index(int(v)) for v in r[2]], np.uint8) for r in recs])
    return dna, header, qual


def test_the_golden_set_is_the_seventeen_archives():
    assert len(EXP) == 17
    modes = {qual_mode_of(AR.read_archive(os.path.join(ARC, n + ".colord"))) for n in EXP}
    assert {0, 4, 5, 6} <= modes                                              # org and the three *-fix archives get the independent qual check below


@pytest.mark.parametrize("name", sorted(EXP))
def test_check_of_a_reference_archive_equals_the_reference_digests(name, decoded):
    r = run_check(os.path.join(ARC, name + ".colord"), name)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no content digest is stored" in r.stdout
    got = parse_check(r.stdout)
    dna, header, qual = reference_triples(name, decoded(name))
    assert got["dna"] == dna
    assert got["header"] == header
    if qual is not None:
        assert got["qual"] == qual
    if name.startswith("bovis24_q_none"):
        assert got["qual"] == (0, 0, 0)


# ---- archives stamped with a `hipdigest` stream ----------------------------------------------------------------------------------------
# one per quality family (org; fix; avg bins, avg and none: dna and header only — their qual digest has its independent check on the GPU),
# the header modes that emit no id, and the stored reference genome
STAMPED = ["bovis24_q_org_balanced", "bovis24_q_4-fix_balanced", "bovis24_q_4-avg_balanced", "bovis24_q_avg_balanced", "bovis24_q_none_balanced",
           "bovis24_header_main", "bovis24_header_none", "c4_ont_genome_stored"]


def stamp(name, path, recs, flip=None, mutate=None):
    """The golden archive `name` with a `hipdigest` stream made from the reference's triples, written to path; flip = (stream, bit) of a sum to flip."""
    arc = AR.read_archive(os.path.join(ARC, name + ".colord"))
    dna, header, qual = reference_triples(name, recs)
    t = {"dna": dna, "qual": qual, "header": header}
    if flip:
        r, s, x = t[flip[0]]
        t[flip[0]] = (r, s, x ^ (1 << flip[1]))
    if mutate:
        mutate(arc)
    payload = R.pack_hipdigest(t["dna"], t["qual"], t["header"])
    assert len(payload) == 80 and R.unpack_hipdigest(payload)["dna"] == t["dna"]
    AR.write_archive(path, list(arc.values()) + [AR.Stream("hipdigest", 0, [(0, payload)])])
    return t


@pytest.mark.parametrize("name", STAMPED)
def test_stamped_archive_decompresses_with_the_ok_line(name, decoded, tmp_path):
    arc, out = str(tmp_path / "s.colord"), str(tmp_path / "o.fastq")
    t = stamp(name, arc, decoded(name))
    r = subprocess.run([CLI, "decompress", arc, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = ", ".join(k for k in ("dna", "qual", "header") if t[k])
    assert f"content digest: ok ({names})" in r.stderr
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == EXP[name]["decompressed_sha256"]
    c = run_check(arc)
    assert c.returncode == 0 and f"content digest: ok ({names})" in c.stdout
    got = parse_check(c.stdout)
    for k in ("dna", "qual", "header"):
        if t[k]:
            assert got["stored " + k] == t[k] == got[k]
    i = subprocess.run([CLI, "info", arc], capture_output=True, text=True)
    assert i.returncode == 0 and "content digest: dna reads=%d" % t["dna"][0] in i.stderr


@pytest.mark.parametrize("name,stream,bit", [("bovis24_q_org_balanced", "dna", 0), ("bovis24_q_org_balanced", "qual", 63), ("bovis24_q_org_balanced", "header", 17),
                                             ("bovis24_q_4-fix_balanced", "qual", 5), ("bovis24_header_none", "header", 40), ("c4_ont_genome_stored", "dna", 31)])
def test_one_flipped_bit_of_a_stored_sum_is_refused(name, stream, bit, decoded, tmp_path):
    arc, out = str(tmp_path / "s.colord"), str(tmp_path / "o.fastq")
    stamp(name, arc, decoded(name), flip=(stream, bit))
    r = subprocess.run([CLI, "decompress", arc, out], capture_output=True, text=True)
    assert r.returncode == 1, r.stderr
    assert "content digest mismatch" in r.stderr and f"stored {stream} reads=" in r.stderr and f"computed {stream} reads=" in r.stderr
    for other in {"dna", "qual", "header"} - {stream}:
        assert f"stored {other} " not in r.stderr
    assert not os.path.exists(out)
    assert run_check(arc).returncode == 1
    r = subprocess.run([CLI, "decompress", "--ignore-digest", arc, out], capture_output=True, text=True)
    assert r.returncode == 0 and "content digest" not in r.stderr
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == EXP[name]["decompressed_sha256"]


def test_corrupt_part_with_a_digest_is_an_error_never_garbage(decoded, tmp_path):
    """The archive of test_decode_cpu.py::test_corrupt_part_is_an_error_not_a_crash — half of the first `dna` part zeroed — with the right digests
    stored: whether the decoder reports a stream error or decodes garbage bases, the exit status is 1 and no output is left."""
    def zero_half(arc):
        meta, payload = arc["dna"].parts[0]
        arc["dna"].parts[0] = (meta, payload[:len(payload) // 2] + bytes(len(payload) - len(payload) // 2))
    name = "bovis24_q_4-avg_balanced"
    arc, out = str(tmp_path / "bad.colord"), str(tmp_path / "o.fastq")
    stamp(name, arc, decoded(name), mutate=zero_half)
    r = subprocess.run([CLI, "decompress", arc, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stderr
    assert "colord_hip:" in r.stderr and not os.path.exists(out)
    assert run_check(arc).returncode == 1


def test_help_names_the_option():
    r = subprocess.run([CLI, "compress-ont", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--digest" in r.stderr and "--ignore-digest" in r.stderr and "colord_hip check" in r.stderr
    r = subprocess.run([CLI, "compress-ont", "--digest", "in.fq"], capture_output=True, text=True)
    assert r.returncode == 1 and "expected input and output paths" in r.stderr and "unknown option" not in r.stderr


# ---- the host code under AddressSanitizer and UBSan, as a program of its own -----------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    """tests/tools/digest_host_test.cpp: csrc/digest.hpp's host loops and the library's decoders (csrc/decode.hip, host code) compiled for the host
    alone with the sanitizers' runtimes linked in; it has its own main and runs as it is, nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("san") / "digest_host_test")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "include"),
                           "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "tools", "digest_host_test.cpp"), "-o", exe])
    return exe


def test_host_loops_under_sanitizers_equal_the_reference(sanitized_program, tmp_path):
    cases = [(0, 0, case_reads()), (0, 1 << 33, case_reads()[:9]), (R.HEADER, 5, case_bytes()), (R.QUAL, 0, case_bytes()), (0, 3, []), (R.QUAL, 3, [b""])]
    cases = [(kind, first, [s if isinstance(s, bytes) else np.asarray(s, np.uint8).tobytes() for s in seqs]) for kind, first, seqs in cases]
    blob = struct.pack("<Q", len(cases))
    for kind, first, seqs in cases:
        off = np.cumsum([0] + [len(s) for s in seqs]).astype("<u8")
        blob += struct.pack("<IQQ", kind, first, len(seqs)) + off.tobytes() + b"".join(seqs)
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    r = subprocess.run([sanitized_program, "cases", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"ok: {len(cases)} cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = [(int(a), int(b), int(c, 16)) for a, b, c in re.findall(r"^case reads=(\d+) symbols=(\d+) sum=0x([0-9a-f]{16})$", r.stdout, re.M)]
    want = [R.digest_bases([np.frombuffer(s, np.uint8) for s in seqs], first) if kind == 0 else R.digest_bytes(kind, seqs, first) for kind, first, seqs in cases]
    assert got == want


@pytest.mark.parametrize("name", ["bovis24_q_org_balanced", "bovis24_q_4-fix_balanced", "bovis24_q_5-avg_balanced", "bovis24_q_2-avg_balanced", "bovis24_q_avg_balanced", "c2_hifi_org"])
def test_digesting_decoder_under_sanitizers(name, sanitized_program, decoded):
    """The quality decoder feeding its symbols into the digest, read by read, over whole archives (first read 2^33): clean under the sanitizers,
    equal to the reference where the symbols follow from the decoded values, and to `colord_hip check` shifted by the first read otherwise."""
    r = subprocess.run([sanitized_program, "decode", os.path.join(ARC, name + ".colord")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok: decoded" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = parse_check(r.stdout)
    recs = decoded(name)
    assert got["dna"] == R.digest_bases([x[1] for x in recs], 1 << 33)
    mode = qual_mode_of(AR.read_archive(os.path.join(ARC, name + ".colord")))
    if mode == 0:
        assert got["qual"] == R.digest_bytes(R.QUAL, [x[2].astype(np.uint8) for x in recs], 1 << 33)
    elif mode in (4, 5, 6):
        vals = R.DEFAULT_D[R.QUAL_MODES[mode]]
        assert got["qual"] == R.digest_bytes(R.QUAL, [np.array([vals.index(int(v)) for v in x[2]], np.uint8) for x in recs], 1 << 33)
    else:                                                                     # counts as `check` reports them: 2 x bins average bytes a read in front of the bases
        chk = parse_check(run_check(os.path.join(ARC, name + ".colord")).stdout)
        assert got["qual"][:2] == chk["qual"][:2] and got["qual"][2] != chk["qual"][2]
