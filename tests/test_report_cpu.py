"""CPU suite of the content report (cl_report, `colord_hip compress-* --report`, `info --report`, `decompress`, `check`).  The
judge is tests/report_ref.py (numpy; the quality values from tests/qual_values_ref.py), first checked against plain Python loops; then the
host functions of the C ABI against it; the reads of the nine reference-written archives with a coded quality stream: the OUT marginal made
from the INPUT alone == the histogram of the quality lines the reference's decompressor returned, base counts and lengths == those of its
decoded records; archives stamped with a `hipreport` stream; the host loops under AddressSanitizer and UBSan as a program of its own.  No
GPU is needed."""
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
import report_ref as P
import test_qual_values_cpu as TC

ROOT, ARC, CLI, EXP, CODED, ALL_MODES = TC.ROOT, TC.ARC, TC.CLI, TC.EXP, TC.CODED, TC.ALL_MODES
CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = _i


def new_report():
    r = N.Report()
    N.load().cl_report_clear(C.byref(r))
    return r


def flat(reads):
    data = np.ascontiguousarray(np.concatenate(reads) if reads else np.zeros(0, np.uint8), dtype=np.uint8)
    off = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    return data, off


def host_report(codes, quals=None, mode=None, T=None, D=None, acc=None):
    """cl_report_bases_host and (with quals) cl_report_quals_host into one report"""
    lib = N.load()
    acc = new_report() if acc is None else acc
    data, off = flat(codes)
    assert lib.cl_report_bases_host(data.ctypes.data, off.ctypes.data, len(codes), C.byref(acc)) == 0
    if quals is not None:
        q, qoff = flat(quals)
        prm = TC.qual_params(mode, T, D)
        assert lib.cl_report_quals_host(C.byref(prm), q.ctypes.data, qoff.ctypes.data, len(quals), C.byref(acc)) == 0
    return acc


def hand_made(seed=2):
    """(codes, input quality bytes) per read: empty, the lengths around a 32-base block, N at positions 0, 31, 32 and last, an all-N read,
    class flags above the code's three bits, qualities outside Phred+33 0..95"""
    rng = np.random.default_rng(seed)
    quals = TC.hand_made_reads(seed)
    quals.append(np.array([0, 32, 33, 128, 129, 255, 40 + 33], np.uint8))
    quals += [(rng.integers(0, 96, L) + 33).astype(np.uint8) for L in (31, 32, 33, 64, 65, 40)]
    codes = [rng.integers(0, 4, len(q)).astype(np.uint8) for q in quals]
    codes[-6][[0, 30]] = 4; codes[-5][[0, 31]] = 4; codes[-4][[31, 32]] = 4; codes[-3][[0, 31, 32, 63]] = 4; codes[-2][64] = 5
    codes[-1][:] = 4
    codes[8] = codes[8] | 0x40                                                 # flag bits are no part of the code
    return codes, quals


# ---- the reference against itself -----------------------------------------------------------------------------------------------------
def test_reference_equals_plain_loops():
    codes, quals = hand_made()
    codes, quals = codes[:9] + codes[-7:], quals[:9] + quals[-7:]               # (the loops are slow: the short reads)
    for mode in ALL_MODES + ["none"]:
        a, b = P.report(codes, quals, mode), P.report_loops(codes, quals, mode)
        assert P.same(a, b) is None and (a["n50"], a["n90"]) == (b["n50"], b["n90"]), (mode, P.same(a, b))
    a = P.report(codes)
    assert P.same(a, P.report_loops(codes)) is None and a["has_qual"] == 0 and not a["q_joint"].any()


def test_reference_simple_values():
    r = P.report([[0, 1, 2, 3, 4, 7, 0]], [np.array([0, 95, 40, 40, 200, 10, 33], np.int64) + 33], "org")
    assert r["base_count"].tolist() == [2, 1, 1, 1, 2] and (r["reads"], r["bases"], r["len_min"], r["len_max"]) == (1, 7, 7, 7)
    assert r["len_hist"][3] == 1 and r["len_bases"][3] == 7
    assert r["q_joint"][40, 40] == 2 and r["q_joint"][0, 0] == 2 and r["q_joint"][95, 95] == 1       # 200 + 33 is no Phred+33 byte of 0..95: 0
    assert r["mean_q_hist"][(95 + 40 + 40 + 10 + 33) // 7] == 1
    r = P.report([[0] * 4], [np.array([0, 6, 7, 95]) + 33], "2-fix")
    assert r["q_joint"][0, 1] == 1 and r["q_joint"][6, 1] == 1 and r["q_joint"][7, 13] == 1 and r["q_joint"][95, 13] == 1
    assert P.nxx([10, 5, 3, 2], 50) == 10 and P.nxx([10, 5, 3, 2], 90) == 3 and P.nxx([4, 4, 2], 50) == 4 and P.nxx([], 50) == 0 and P.nxx([0, 0], 50) == 0
    assert P.nxx([5, 5], 50) == 5 and P.nxx([6, 4], 60) == 6 and P.nxx([6, 4], 61) == 4
    e = P.empty()
    assert e["len_min"] == (1 << 64) - 1 and P.same(P.add(e, r), r) is None
    L = P.loss(r)
    assert L["max_abs"] == 82 and abs(L["unchanged"]) == 0 and abs(L["mae"] - (1 + 5 + 6 + 82) / 4) < 1e-12


# ---- the host functions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ALL_MODES + ["none"])
def test_host_report_equals_the_reference(mode):
    codes, quals = hand_made()
    cases = [(None, None)]
    if mode[0] in "245":
        n = int(mode[0])
        cases.append(([5] * 2 + list(range(30, 30 + n - 3)) if n > 2 else [0], list(range(40, 40 + n)) if mode.endswith("fix") else None))      # an empty bin; custom -D
        cases.append((list(range(10, 10 + n - 2)) + [96], [0, 95, 7, 9, 11][:n] if mode.endswith("fix") else None))                               # -T ending at 96; -D at its limits
    for T, D in cases:
        got = host_report(codes, quals, mode, T, D).as_dict()
        want = P.report(codes, quals, mode, T, D)
        assert P.same(got, want) is None, (mode, T, D, P.same(got, want))
        cut = 9                                                               # two calls over the halves, into one report and added from two
        acc = host_report(codes[cut:], quals[cut:], mode, T, D)
        assert P.same(host_report(codes[:cut], quals[:cut], mode, T, D, acc).as_dict(), want) is None
        a, b = host_report(codes[:cut], quals[:cut], mode, T, D), host_report(codes[cut:], quals[cut:], mode, T, D)
        N.load().cl_report_add(C.byref(a), C.byref(b))
        assert P.same(a.as_dict(), want) is None
    if mode == "none":
        assert want["has_qual"] == 0 and got["q_reads"] == 0 and not got["q_joint"].any()


def test_host_values_report_is_the_out_marginal():
    lib = N.load()
    _, quals = hand_made()
    for mode in ALL_MODES:
        values = TC.host_values(mode, quals)
        q, off = flat(values)
        acc = new_report()
        assert lib.cl_report_values_host(q.ctypes.data, off.ctypes.data, len(values), C.byref(acc)) == 0
        got, want = acc.as_dict(), P.report([np.zeros(len(x), np.uint8) for x in quals], quals, mode)
        assert np.array_equal(got["q_joint"][0], P.out_marginal(want)) and not got["q_joint"][1:].any(), mode
        assert (got["q_reads"], got["q_symbols"], got["has_qual"], got["reads"]) == (want["q_reads"], want["q_symbols"], 1, 0)
        assert P.same(got, P.values_report(values)) is None


def test_host_refuses_what_it_cannot_count_and_clear_is_the_empty_report():
    lib = N.load()
    off = np.zeros(2, np.uint64); acc = new_report()
    assert P.same(acc.as_dict(), P.empty()) is None
    for p in (TC.qual_params("2-fix", D=[1]), TC.qual_params("2-fix", D=[1, 96]), TC.qual_params("4-avg", T=[7, 14])):
        assert lib.cl_report_quals_host(C.byref(p), None, off.ctypes.data, 1, C.byref(acc)) == N.CL_E_INVALID
    assert P.same(acc.as_dict(), P.empty()) is None                            # a refused call adds nothing
    assert lib.cl_report_bases_host(None, off.ctypes.data, 1, None) == N.CL_E_INVALID
    assert lib.cl_report_values_host(None, off.ctypes.data, 1, None) == N.CL_E_INVALID
    p = TC.qual_params("2-fix", D=[1, 95])
    assert lib.cl_report_quals_host(C.byref(p), None, off.ctypes.data, 1, C.byref(acc)) == 0 and acc.q_reads == 1 and acc.has_qual == 1


def test_binding_declares_the_new_entry_points():
    lib = N.load()
    for name in ("cl_report_clear", "cl_report_add", "cl_report_bases", "cl_report_quals", "cl_report_bases_host", "cl_report_quals_host", "cl_report_values_host",
                 "cl_ctx_set_report", "cl_ctx_report", "cl_compressor_report"):
        assert name in N.exported_names() and hasattr(lib, name)
    from colord_amd import device as D
    for name in ("set_report", "report", "report_bases", "report_quals"):
        assert hasattr(D.Context, name)
    assert hasattr(D.Compressor, "report")
    assert C.sizeof(N.Report) == 8 * (2 + 5 + 2 + 66 + 3 + 96 + 96 * 96)


# ---- the golden archives -----------------------------------------------------------------------------------------------------------------
def input_records(n=24):
    """(codes, quality bytes) of the first n reads of tests/data/M.bovis.fastq.gz: what the reference compressed"""
    lines = gzip.open(os.path.join(ROOT, "tests", "data", "M.bovis.fastq.gz"), "rb").read().split(b"\n")
    return [CODE[np.frombuffer(lines[4 * i + 1], np.uint8)] for i in range(n)], [np.frombuffer(lines[4 * i + 3], np.uint8) for i in range(n)]


@pytest.fixture(scope="module")
def golden_input():
    return input_records()


@pytest.fixture(scope="module")
def wanted(golden_input):
    """name -> report_ref of the INPUT under the archive's mode (computed once)"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = P.report(golden_input[0], golden_input[1], CODED[name])
        return cache[name]
    return get


decoded = TC.decoded


@pytest.mark.parametrize("mode", ALL_MODES + ["none"])
def test_host_report_of_the_golden_input_equals_the_reference_in_every_mode(mode, golden_input):
    codes, quals = golden_input
    got, want = host_report(codes, quals, mode).as_dict(), P.report(codes, quals, mode)
    assert P.same(got, want) is None, (mode, P.same(got, want))
    assert got["reads"] == 24 and got["bases"] == sum(len(c) for c in codes)


@pytest.mark.parametrize("name", sorted(CODED))
def test_report_of_the_input_is_what_the_reference_archive_decodes_to(name, decoded, golden_input, wanted):
    codes, quals = golden_input
    recs = decoded(name)                                                       # (id, codes, phred, plus) as the pinned decompressor returned them
    got = host_report(codes, quals, CODED[name]).as_dict()
    assert P.same(got, wanted(name)) is None, P.same(got, wanted(name))
    hist = np.bincount(np.concatenate([r[2] for r in recs]).astype(np.int64), minlength=96).astype(np.uint64)
    assert np.array_equal(P.out_marginal(got), hist)                          # OUT marginal from the INPUT alone == the reference's quality lines
    dec = P.report([r[1] for r in recs])
    assert P.same(got, dec, ("reads", "bases", "base_count", "len_min", "len_max", "len_hist", "len_bases")) is None
    assert (wanted(name)["n50"], wanted(name)["n90"]) == (dec["n50"], dec["n90"])
    if CODED[name] == "org":
        assert P.loss(got)["unchanged"] == 1.0 and np.array_equal(P.in_marginal(got), hist)


# ---- the stream --------------------------------------------------------------------------------------------------------------------------
def test_stream_round_trip_in_the_reference():
    codes, quals = hand_made()
    for mode in ("4-avg", "org", "none"):
        r = P.report(codes, quals, mode)
        b = P.pack_hipreport(r)
        back = P.unpack_hipreport(b)
        assert P.same(back, r) is None and (back["n50"], back["n90"]) == (r["n50"], r["n90"]) and P.pack_hipreport(back) == b
        assert len(b) == 8 + 77 * 8 + ((98 * 8 + 4 + 10 * int(np.count_nonzero(r["q_joint"]))) if r["has_qual"] else 0)


def stamp(name, path, payload, extra=()):
    arc = AR.read_archive(os.path.join(ARC, name + ".colord"))
    AR.write_archive(path, list(arc.values()) + [AR.Stream("hipreport", 0, [(0, payload)])] + list(extra))


STAMPED = ["bovis24_q_4-avg_balanced", "bovis24_q_5-fix_balanced"]


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


@pytest.mark.parametrize("name", STAMPED)
def test_stamped_archive_passes_check_decompress_and_info(name, wanted, tmp_path):
    arc, out = str(tmp_path / "s.colord"), str(tmp_path / "o.fastq")
    want = wanted(name)
    stamp(name, arc, P.pack_hipreport(want))
    r = run("decompress", arc, out)
    assert r.returncode == 0 and "content report: ok" in r.stderr, r.stderr
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == EXP[name]["decompressed_sha256"]
    c = run("check", arc)
    assert c.returncode == 0 and "content report: ok" in c.stdout, c.stdout
    i = run("info", arc)
    assert i.returncode == 0 and "content report: 24 reads, %d bases, N50 %d" % (want["bases"], want["n50"]) in i.stderr
    j = run("info", "--report", "--json", arc)
    assert j.returncode == 0, j.stderr
    o = json.loads(j.stdout)
    got = P.empty()
    for k in P.FIELDS:
        if k != "q_joint":
            got[k] = np.array(o[k], np.uint64) if isinstance(o[k], list) else o[k]
    for a, b, n in o["q_joint"]:
        got["q_joint"][a, b] = n
    assert P.same(got, want) is None and (o["n50"], o["n90"], o["version"]) == (want["n50"], want["n90"], 1)
    L = P.loss(want)
    assert abs(o["mae"] - L["mae"]) < 1e-8 and abs(o["rmse"] - L["rmse"]) < 1e-8 and abs(o["unchanged"] - L["unchanged"]) < 1e-8 and o["max_abs"] == L["max_abs"]
    t = run("info", "--report", arc)
    assert t.returncode == 0 and "arithmetic mean of the Phred values" in t.stdout and "N50 %d, N90 %d" % (want["n50"], want["n90"]) in t.stdout
    assert ("MAE %.4f" % L["mae"]) in t.stdout and ("max |delta| %d" % L["max_abs"]) in t.stdout


def tampered(want, what):
    """one counter off per field class -> (report, the text that must name it)"""
    r = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want.items()}
    if what == "base_count":
        r["base_count"][2] += np.uint64(1)
        return r, "base count G: stored %s, decoded %s" % (spaced(int(r["base_count"][2])), spaced(int(want["base_count"][2])))
    if what == "len_bin":
        b = int(np.nonzero(want["len_hist"])[0][0])
        r["len_hist"][b] += np.uint64(1)
        return r, "reads of length bin %d: stored %s, decoded %s" % (b, spaced(int(r["len_hist"][b])), spaced(int(want["len_hist"][b])))
    if what == "n50":
        r["n50"] += 1
        return r, "N50: stored %s, decoded %s" % (spaced(r["n50"]), spaced(want["n50"]))
    i, j = [int(x[0]) for x in np.nonzero(want["q_joint"])]
    k = int(np.nonzero(want["q_joint"][i])[0][-1])                           # one base moved between two OUT values of the same input quality: every total stays
    assert k != j
    r["q_joint"][i, j] -= np.uint64(1); r["q_joint"][i, k] += np.uint64(1)
    lo = min(j, k)
    return r, "quality value %d: stored %s, decoded %s" % (lo, spaced(int(P.out_marginal(r)[lo])), spaced(int(P.out_marginal(want)[lo])))


def spaced(x):
    return f"{x:,}".replace(",", " ")


@pytest.mark.parametrize("what", ["base_count", "len_bin", "n50", "out_value"])
def test_a_tampered_counter_is_refused_and_exactly_it_is_named(what, wanted, tmp_path):
    name = STAMPED[0]
    arc, out = str(tmp_path / "s.colord"), str(tmp_path / "o.fastq")
    bad, text = tampered(wanted(name), what)
    stamp(name, arc, P.pack_hipreport(bad))
    r = run("decompress", arc, out)
    assert r.returncode == 1 and "content report mismatch" in r.stderr and text in r.stderr, (text, r.stderr)
    assert r.stderr.count("stored ") == 1 and not os.path.exists(out)
    c = run("check", arc)
    assert c.returncode == 1 and ("content report mismatch: " + text) in c.stdout, c.stdout
    r = run("decompress", "--ignore-digest", arc, out)
    assert r.returncode == 0 and "content report" not in r.stderr
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == EXP[name]["decompressed_sha256"]


def test_the_in_side_is_not_checked(wanted, tmp_path):
    """the input side cannot be recomputed from a lossy archive: a base moved between two INPUT qualities of one stored value passes"""
    name = STAMPED[0]
    want = wanted(name)
    r = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want.items()}
    j = int(np.nonzero(P.out_marginal(want))[0][0])
    rows = np.nonzero(want["q_joint"][:, j])[0]
    assert len(rows) >= 2
    r["q_joint"][rows[0], j] -= np.uint64(1); r["q_joint"][rows[1], j] += np.uint64(1)
    arc = str(tmp_path / "s.colord")
    stamp(name, arc, P.pack_hipreport(r))
    c = run("check", arc)
    assert c.returncode == 0 and "content report: ok" in c.stdout


@pytest.mark.parametrize("how", ["version_2", "one_byte_short", "one_byte_more", "cell_out_of_order", "header_only"])
def test_a_stream_of_another_shape_is_refused_cleanly(how, wanted, tmp_path):
    name = STAMPED[0]
    arc, out = str(tmp_path / "s.colord"), str(tmp_path / "o.fastq")
    good = P.pack_hipreport(wanted(name))
    cells = 8 + 77 * 8 + 98 * 8 + 4
    payload = {"version_2": struct.pack("<I", 2) + good[4:], "one_byte_short": good[:-1], "one_byte_more": good + b"\0",
               "cell_out_of_order": good[:cells] + good[cells + 10:cells + 20] + good[cells:cells + 10] + good[cells + 20:], "header_only": good[:8]}[how]
    stamp(name, arc, payload)
    r = run("decompress", arc, out)
    assert r.returncode == 1 and "`hipreport` stream is not one this build reads" in r.stderr and not os.path.exists(out)
    c = run("check", arc)
    assert c.returncode == 1 and "`hipreport` stream is not one this build reads" in c.stdout
    i = run("info", "--report", arc)
    assert i.returncode == 1 and "is not one this build reads" in i.stderr
    r = run("decompress", "--ignore-digest", arc, out)
    assert r.returncode == 0 and os.path.exists(out)


@pytest.mark.parametrize("name", ["bovis24_q_4-avg_balanced", "bovis24_q_none_balanced"])
def test_an_archive_without_the_stream_behaves_as_before_and_check_prints_what_it_decodes(name, golden_input, tmp_path):
    arc, out = os.path.join(ARC, name + ".colord"), str(tmp_path / "o.fastq")
    r = run("decompress", arc, out)
    assert r.returncode == 0 and "content report" not in r.stderr
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == EXP[name]["decompressed_sha256"]
    i = run("info", arc)
    assert i.returncode == 0 and "content report" not in i.stderr
    i = run("info", "--report", arc)
    assert i.returncode == 1 and "no content report is stored" in i.stderr
    c = run("check", arc)
    assert c.returncode == 0 and "no content report is stored in this archive" in c.stdout
    want = P.report(golden_input[0])
    assert "reads: 24\nbases: %d\n" % want["bases"] in c.stdout and "N50 %d, N90 %d" % (want["n50"], want["n90"]) in c.stdout
    assert "base composition: A %d, C %d, G %d, T %d, N %d;" % tuple(int(x) for x in want["base_count"]) in c.stdout
    if name.endswith("none_balanced"):
        assert "qualities: none" in c.stdout
    else:
        m = P.out_marginal(P.report(golden_input[0], golden_input[1], "4-avg"))
        listed = {int(a): int(b) for a, b in re.findall(r"^  ([ \d]\d)  (\d+)$", c.stdout.split("quality values (value: decoded):")[1], re.M)}
        assert listed == {int(q): int(m[q]) for q in np.nonzero(m)[0]}


def test_a_fasta_report_has_no_quality_part(golden_input, tmp_path):
    name = "bovis24_q_none_balanced"
    want = P.report(golden_input[0])
    arc = str(tmp_path / "s.colord")
    stamp(name, arc, P.pack_hipreport(want))
    assert len(P.pack_hipreport(want)) == 8 + 77 * 8
    c = run("check", arc)
    assert c.returncode == 0 and "content report: ok" in c.stdout, c.stdout
    j = run("info", "--report", "--json", arc)
    assert j.returncode == 0 and json.loads(j.stdout)["has_qual"] == 0 and "q_joint" not in json.loads(j.stdout)


def test_help_names_the_option():
    r = run("compress-ont", "--help")
    assert r.returncode == 0 and "--report" in r.stderr and "hipreport" in r.stderr and "NOT the error-probability mean" in r.stderr
    assert "is not checked" in r.stderr and "info [--report [--json]]" in r.stderr
    r = run("compress-ont", "--report", "in.fq")
    assert r.returncode == 1 and "expected input and output paths" in r.stderr and "unknown option" not in r.stderr


# ---- the host loops under AddressSanitizer and UBSan, as a program of its own ------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    """tests/tools/report_host_test.cpp: csrc/report.hpp and csrc/cli/report_stream.hpp under a host compiler alone (they need no HIP), the
    sanitizers' runtimes linked in; it has its own main and runs as it is, nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("san") / "report_host_test")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "report_host_test.cpp"), "-o", exe])
    return exe


def test_host_loops_under_sanitizers_equal_the_reference(sanitized_program, tmp_path):
    codes, quals = hand_made(seed=6)
    cases = [(m, None, None, codes, quals) for m in ALL_MODES + ["none"]]
    cases += [("4-avg", [5, 5, 30], None, codes, quals), ("5-fix", [3, 9, 9, 96], [0, 95, 7, 9, 11], codes, quals), ("avg", None, None, [], []),
              ("2-avg", None, None, [np.zeros(0, np.uint8)], [np.zeros(0, np.uint8)])]
    blob = struct.pack("<Q", len(cases))
    for mode, T, D, cd, ql in cases:
        p = TC.qual_params(mode, T, D)
        off = np.cumsum([0] + [len(r) for r in cd]).astype("<u8")
        blob += struct.pack("<iI8II8IQ", p.mode, p.n_fwd, *p.fwd, p.n_rev, *p.rev, len(cd)) + off.tobytes() + b"".join(r.tobytes() for r in cd) + b"".join(r.tobytes() for r in ql)
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    r = subprocess.run([sanitized_program, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"ok: {len(cases)} cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = re.findall(r"^case ([0-9a-f]*)$", r.stdout, re.M)
    assert len(got) == len(cases)
    for (mode, T, D, cd, ql), hexv in zip(cases, got):
        assert bytes.fromhex(hexv) == P.pack_hipreport(P.report(cd, ql, mode, T, D)), (mode, T)
