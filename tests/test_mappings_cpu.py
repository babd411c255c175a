"""CPU suite of the read-to-genome mappings (`colord_hip compress-* -G genome --mappings`, `info --mappings`).  The judge is
tests/mappings_ref.py (plain Python, written from the definition).  Here: the host twin of the lift (cl_mappings_lift_host) equals the judge on the
constructed geometries and records of tests/mappingcases.py, refuses what the judge refuses and writes nothing then; the ABI; the `hipmappings`
stream through `info --mappings` as PAF, as a coverage track and as a summary, and every refusal of its reader; the options; the sequence names of
a FASTA; the host twin and the stream's code under AddressSanitizer and UBSan as a program of its own.  No GPU is needed."""
import ctypes as C
import json
import os
import re
import struct
import subprocess
import numpy as np
import pytest
from colord_amd import _native as N, archive as AR
import overlaps_ref as OR
import mappings_ref as MR
import mappingcases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
GOLDEN_ARC = os.path.join(ROOT, "tests", "golden", "archives", "bovis24_q_4-avg_balanced.colord")


def host_lift(recs, geo, cap=None):
    """cl_mappings_lift_host -> (status, (m, 12) uint32 records, n_out, bad record, bad code); cap None: the need is asked for first"""
    lib = N.load()
    recs = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, 12)
    sl = np.ascontiguousarray(geo["seq_len"], dtype=np.uint64)
    bad, code, n = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    args = (recs.ctypes.data if len(recs) else None, len(recs), sl.ctypes.data if len(sl) else None, len(sl), geo["read_len"], geo["overlap"])
    if cap is None:
        st = lib.cl_mappings_lift_host(*args, None, 0, C.byref(n), C.byref(bad), C.byref(code))
        if st not in (N.CL_OK, N.CL_E_CAPACITY):
            return st, np.zeros((0, 12), np.uint32), n.value, bad.value, code.value
        cap = n.value
    out = np.full((cap + 1, 12), 0xabababab, np.uint32)       # one record more than asked for: it must stay as it is
    st = lib.cl_mappings_lift_host(*args, out.ctypes.data, cap, C.byref(n), C.byref(bad), C.byref(code))
    assert (out[cap] == 0xabababab).all()
    if st != N.CL_OK:
        assert (out == 0xabababab).all(), "something was written although the call failed"
    return st, out[:n.value if st == N.CL_OK else 0].copy(), n.value, bad.value, code.value


# ---- the geometry and the host twin against the judge -----------------------------------------------------------------------------------
def test_the_constructed_geometry_has_every_shape():
    P = MR.pieces(**MC.NINE)
    per = [[p for p in P if p[0] == s] for s in range(9)]
    assert [len(x) for x in per] == [4, 0, 1, 2, 3, 3, 1, 5, 1] and len(P) == 20
    assert per[4][-1] == (4, 140, 1) and per[4][-1][2] < MC.NINE["overlap"] and per[3][-1][2] == MC.NINE["overlap"] and per[2] == [(2, 0, 70)]
    assert [len([p for p in MR.pieces(**MC.ONE)])] == [4] and MR.pieces(**MC.ONE)[-1] == (0, 750, 250)


@pytest.mark.parametrize("geo", sorted(MC.GEOMETRIES))
@pytest.mark.parametrize("mode", MC.MODES)
def test_host_twin_equals_the_judge(geo, mode):
    G = MC.GEOMETRIES[geo]
    for n in MC.SIZES:
        recs = MC.records(G, n, mode)
        want = MR.lift(recs, **G)
        st, got, m, _, _ = host_lift(recs, G)
        assert st == 0 and m == len(want) and np.array_equal(got, want), (geo, mode, n)
        assert len(want) == {"none_dropped": n, "all_dropped": 0, "alternating": n // 2}[mode]
        if len(want):
            st, none, m, _, _ = host_lift(recs, G, cap=len(want) - 1)                       # the capacity protocol: the need, nothing written
            assert st == N.CL_E_CAPACITY and m == len(want) and len(none) == 0


def test_the_lift_moves_what_it_should_and_nothing_else():
    recs = MC.records(MC.NINE, 257, "none_dropped")
    got = MR.lift(recs, **MC.NINE)
    P = MR.pieces(**MC.NINE)
    f, g = ({k: r[:, i].astype(np.int64) for i, k in enumerate(MR.FIELDS)} for r in (recs, got))
    start = np.array([P[t][1] for t in f["t"]]); seq = np.array([P[t][0] for t in f["t"]])
    assert (g["t"] == seq).all() and (g["ts"] == f["ts"] + start).all() and (g["te"] == f["te"] + start).all() and (g["tlen"] == np.array(MC.NINE["seq_len"])[seq]).all()
    assert (g["flags"] == f["flags"] | MR.GENOME).all() and set(f["flags"].tolist()) == {0, 1, 2, 3}
    for k in ("q", "qlen", "qs", "qe", "matches", "subst", "anchor_bases"):
        assert (g[k] == f[k]).all()
    assert set(f["t"].tolist()) == set(range(len(P))) and (g["te"] <= g["tlen"]).all() and set(seq.tolist()) == {0, 2, 3, 4, 5, 6, 7, 8}
    edge = MC.records(MC.NINE, 4, "alternating")                                        # t = n_pseudo is a read, t = n_pseudo - 1 the last piece
    assert edge[0, 1] == len(P) and edge[1, 1] == len(P) - 1 and len(MR.lift(edge, **MC.NINE)) == 2


@pytest.mark.parametrize("name", ["tlen", "position", "end"])
def test_a_record_that_cannot_be_lifted_is_refused_and_nothing_is_written(name):
    recs, first, code = MC.refused()[name]
    with pytest.raises(MR.Refused) as x:
        MR.lift(recs, **MC.NINE)
    assert (x.value.record, x.value.code) == (first, code)
    for cap in (None, 1000):
        st, _, n, bad, c = host_lift(recs, MC.NINE, cap)
        assert st == N.CL_E_INVALID and n == 0 and bad == first and c == code


def test_geometries_that_are_refused():
    recs = MC.records(MC.ONE, 3, "none_dropped")
    assert host_lift(recs, dict(seq_len=[1000], read_len=50, overlap=50))[0] == N.CL_E_INVALID
    assert host_lift(recs, dict(seq_len=[1000], read_len=10, overlap=50))[0] == N.CL_E_INVALID
    assert host_lift(recs, dict(seq_len=[1 << 32], read_len=300, overlap=50))[0] == N.CL_E_UNSUPPORTED
    assert host_lift(np.zeros((0, 12), np.uint32), dict(seq_len=[(1 << 32) - 1], read_len=300, overlap=50))[0] == N.CL_OK
    st, got, n, _, _ = host_lift(recs, dict(seq_len=[], read_len=300, overlap=50))         # no sequence: every record names a read
    assert st == 0 and n == 0


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
NAMES = ["cl_mappings_lift", "cl_mappings_lift_host", "cl_ctx_set_mappings", "cl_ctx_mappings", "cl_compressor_mappings", "cl_compressor_genome_geometry"]


def test_abi_names():
    header = open(os.path.join(ROOT, "include", "colord_hip.h")).read()
    lib = N.load()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in N.exported_names() and hasattr(lib, n)
    from colord_amd import device as D
    for name in ("set_mappings", "mappings", "mappings_lift"):
        assert hasattr(D.Context, name)
    assert hasattr(D.Compressor, "mappings") and hasattr(D.Compressor, "genome_geometry")
    for n in ("cl_mappings_lift_host", "cl_ctx_set_mappings", "cl_ctx_mappings", "cl_compressor_mappings"):
        assert n in D._OrderedLib._HOST_ONLY
    assert "read-to-genome mappings (DESIGN.md 4m" in header and "not stitched" in header


# ---- the stream through `info` -----------------------------------------------------------------------------------------------------------
def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def stamp(path, payload):
    arc = AR.read_archive(GOLDEN_ARC)
    AR.write_archive(path, list(arc.values()) + [AR.Stream("hipmappings", 0, [(0, payload)])])


SEQ_NAMES = ["chrA", "empty", "", "chr3", "chr4", "chr5", "one", "chr7", "last|x"]        # (a sequence without a name is printed by its index)


@pytest.fixture(scope="module")
def hand_built(tmp_path_factory):
    """lifted records over the 24 reads of a golden archive, so that --names finds every id"""
    recs = MC.records(MC.NINE, 60, "none_dropped", seed=9)
    recs[:, 0] = np.sort(np.random.default_rng(4).integers(0, 24, len(recs)))
    lifted = MR.lift(recs, **MC.NINE)
    arc = str(tmp_path_factory.mktemp("map") / "m.colord")
    stamp(arc, MR.pack(lifted, MC.NINE["seq_len"], SEQ_NAMES, 100, 30))
    return arc, lifted


def test_pack_and_parse_round_trip(hand_built):
    _, lifted = hand_built
    b = MR.pack(lifted, MC.NINE["seq_len"], SEQ_NAMES, 100, 30)
    sl, names, rl, ov, recs = MR.parse(b)
    assert (sl, names, rl, ov) == (MC.NINE["seq_len"], SEQ_NAMES, 100, 30) and np.array_equal(recs, lifted)
    assert len(b) == 28 + sum(10 + len(n) for n in SEQ_NAMES) + 48 * len(lifted)


def test_info_prints_paf_coverage_and_summary(hand_built, tmp_path):
    arc, lifted = hand_built
    sl = MC.NINE["seq_len"]
    r = run("info", "--mappings", arc)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == MR.paf_lines(lifted, sl, SEQ_NAMES)
    cols = [line.split("\t") for line in r.stdout.splitlines()]
    assert all(len(c) == 15 and c[11] == "255" and c[5] in SEQ_NAMES + ["2"] and int(c[6]) == sl[(SEQ_NAMES + ["2"]).index(c[5]) if c[5] != "2" else 2] for c in cols)
    assert {c[5] for c in cols} >= {"chrA", "2", "last|x"}
    blocks = sorted(OR.block(x) for x in lifted)
    mid = blocks[len(blocks) // 2]
    r = run("info", "--mappings", "--min-block", str(mid), arc)
    assert r.returncode == 0 and r.stdout.splitlines() == MR.paf_lines(lifted, sl, SEQ_NAMES, min_block=mid) and 0 < len(r.stdout.splitlines()) < len(lifted)
    dec = str(tmp_path / "d.fastq")
    assert run("decompress", arc, dec).returncode == 0                                  # `decompress` ignores the stream ...
    assert run("decompress", GOLDEN_ARC, str(tmp_path / "o.fastq")).returncode == 0
    assert open(dec).read() == open(str(tmp_path / "o.fastq")).read()
    ids = [line[1:].split()[0] for line in open(dec).read().splitlines()[0::4]]
    r = run("info", "--mappings", "--names", arc)
    assert r.returncode == 0 and len(ids) == 24 and r.stdout.splitlines() == MR.paf_lines(lifted, sl, SEQ_NAMES, read_names=ids)
    assert run("check", arc).returncode == 0                                            # ... and so does `check`
    for w in (1, 7, 64, 100, 1000):
        r = run("info", "--mappings", "--coverage", str(w), arc)
        assert r.returncode == 0 and r.stdout.splitlines() == MR.coverage_lines(lifted, sl, SEQ_NAMES, w), w
        rows = [line.split("\t") for line in r.stdout.splitlines()]
        assert len(rows) == sum(-(-ln // w) for ln in sl) and "empty" not in {x[0] for x in rows}
        total = sum(round(float(x[3]) * (int(x[2]) - int(x[1]))) for x in rows)
        assert total == int((lifted[:, 7].astype(np.int64) - lifted[:, 6]).sum())
        assert all(int(x[2]) - int(x[1]) == w or int(x[2]) == sl[(SEQ_NAMES + ["2"]).index(x[0]) if x[0] != "2" else 2] for x in rows)       # only a sequence's last window is short
    r = run("info", "--mappings", "--summary", "--json", arc)
    assert r.returncode == 0 and json.loads(r.stdout) == MR.summary(lifted, 24)
    s = json.loads(r.stdout)
    assert s["forward"] > 0 and s["reverse"] > 0 and sum(s["identity_hist"]) == s["records"] == len(lifted) and 0 < s["reads_mapped"] <= 24
    r = run("info", "--mappings", "--summary", arc)
    assert r.returncode == 0 and "reads in the archive: 24" in r.stdout and "records: %d" % len(lifted) in r.stdout and "reads with a mapping: %d" % s["reads_mapped"] in r.stdout
    i = run("info", arc)
    assert i.returncode == 0 and "mappings: %d records" % len(lifted) in i.stderr and "9 sequences" in i.stderr
    plain = run("info", GOLDEN_ARC)
    assert plain.returncode == 0 and "mappings" not in plain.stderr
    none = run("info", "--mappings", GOLDEN_ARC)
    assert none.returncode == 1 and "no mappings are stored" in none.stderr
    empty = str(tmp_path / "e.colord")
    stamp(empty, MR.pack(np.zeros((0, 12), np.uint32), sl, SEQ_NAMES, 100, 30))
    r = run("info", "--mappings", empty)
    assert r.returncode == 0 and r.stdout == ""
    r = run("info", "--mappings", "--coverage", "100", empty)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == sum(-(-ln // 100) for ln in sl) and all(line.endswith("\t0.000000") for line in r.stdout.splitlines())
    far = lifted[:1].copy(); far[0, 0] = 30                                                # read 30 of 24
    stamp(empty, MR.pack(far, sl, SEQ_NAMES, 100, 30))
    r = run("info", "--mappings", "--names", empty)
    assert r.returncode == 1 and "names a read" in r.stderr


def bad_payloads():
    recs = MR.lift(MC.records(MC.NINE, 5, "none_dropped"), **MC.NINE)
    sl = MC.NINE["seq_len"]
    good = MR.pack(recs, sl, SEQ_NAMES, 100, 30)
    table_end = len(good) - 48 * len(recs)
    t_out, te_out = recs.copy(), recs.copy()
    t_out[2, 1] = 9
    te_out[4, 7] = sl[te_out[4, 1]] + 1
    long_name = bytearray(good); struct.pack_into("<H", long_name, 28 + 8, 60000)
    return {"version_2": MR.pack(recs, sl, SEQ_NAMES, 100, 30, version=2), "record_size_44": MR.pack(recs, sl, SEQ_NAMES, 100, 30, record_bytes=44), "one_byte_short": good[:-1],
            "one_record_short": good[:-48], "count_one_more": MR.pack(recs, sl, SEQ_NAMES, 100, 30, count=6), "head_cut": good[:20], "name_table_cut": good[:table_end - 3],
            "name_longer_than_the_stream": bytes(long_name), "one_sequence_more": good[:8] + struct.pack("<I", 10) + good[12:], "sequences_without_bytes": good[:8] + struct.pack("<I", 0xffffffff) + good[12:],
            "target_outside_the_table": MR.pack(t_out, sl, SEQ_NAMES, 100, 30), "end_behind_the_sequence": MR.pack(te_out, sl, SEQ_NAMES, 100, 30)}


@pytest.mark.parametrize("how", sorted(bad_payloads()))
def test_a_stream_of_another_shape_is_refused_cleanly(how, tmp_path):
    payload = bad_payloads()[how]
    with pytest.raises(ValueError):
        MR.parse(payload)
    arc = str(tmp_path / "s.colord")
    stamp(arc, payload)
    for mode in ([], ["--coverage", "10"], ["--summary"]):
        r = run("info", "--mappings", *mode, arc)
        assert r.returncode == 1 and "`hipmappings` stream is not one this build reads" in r.stderr and r.stdout == ""
    i = run("info", arc)
    assert i.returncode == 0 and "a `hipmappings` stream this build cannot read" in i.stderr


def test_help_and_refused_combinations(tmp_path):
    r = run("compress-ont", "--help")
    assert r.returncode == 0 and "--mappings" in r.stderr and "hipmappings" in r.stderr and "YIELDS NO RECORD" in r.stderr and "NOT STITCHED" in r.stderr
    assert "info --mappings [--min-block N] [--names] | --mappings --coverage W | --mappings --summary [--json] archive.colord" in r.stderr
    out = str(tmp_path / "out.colord")
    for extra, text in (([], "--mappings needs a reference genome (-G)"), (["-G", "genome.fa", "--gpus", "2"], "--mappings is not available with --gpus > 1"),
                        (["-G", "genome.fa", "--domains", "2"], "--mappings is not available with --domains > 1"), (["-G", "genome.fa", "--overlaps"], "--mappings is not available with --overlaps")):
        r = run("compress-ont", "--mappings", *extra, "in.fq", out)
        assert r.returncode == 1 and text in r.stderr and not os.path.exists(out), r.stderr
    for args in (["--coverage", "10"], ["--summary"], ["--mappings", "--coverage", "10", "--summary"], ["--mappings", "--json"], ["--mappings", "--coverage", "10", "--names"],
                 ["--mappings", "--summary", "--min-block", "3"], ["--mappings", "--report"], ["--mappings", "--overlaps"], ["--mappings", "--coverage", "10", "--json"]):
        r = run("info", *args, GOLDEN_ARC)
        assert r.returncode == 1 and "usage" in r.stderr, args
    for args in (["--mappings", "--coverage", "0"], ["--mappings", "--coverage", "x"], ["--mappings", "--coverage"]):
        r = run("info", *args, GOLDEN_ARC)
        assert r.returncode == 1 and "--coverage needs a window length" in r.stderr, args


# ---- the FASTA's sequence names ---------------------------------------------------------------------------------------------------------
def test_sequence_names_are_indexed_as_the_sequences(tmp_path):
    """genome_io::read_fasta_names next to genome_io::read_fasta on one FASTA (the compress command needs a GPU, so the two readers are compiled
    here into a program of their own, under the sanitizers): as many names as sequences, in the same order, whatever the lines look like"""
    src = tmp_path / "names.cpp"
    src.write_text('#include "%s"\n#include <cstdio>\nint main(int, char** v) { const auto S = genome_io::read_fasta(v[1]); const auto N = genome_io::read_fasta_names(v[1]);\n'
                   'printf("%%zu %%zu\\n", S.off.size() - 1, N.size()); for (size_t i = 0; i < N.size(); ++i) printf("%%s\\t%%llu\\n", N[i].c_str(), (unsigned long long)(S.off[i + 1] - S.off[i])); return 0; }\n'
                   % os.path.join(ROOT, "colord_amd", "csrc", "cli", "genome_io.hpp"))
    exe = str(tmp_path / "names")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", str(src), "-o", exe, "-lz"])
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">chr1 first sequence\nACGT\nACNNGT\n>empty\tnothing kept\nNNNN\n>chr3\r\nAC\r\n\r\n>\nGG\n>tail|7 x\n>not_a_header\nA>C\nT")
    r = subprocess.run([exe, str(fa)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    # (a `>` line right behind a header line is sequence text to read_fasta: `not_a_header` gives its A, C, G, T letters to `tail|7`)
    assert lines[0] == "5 5" and lines[1:] == ["chr1\t8", "empty\t0", "chr3\t2", "\t2", "tail|7\t%d" % (sum(c in "ACGTacgt" for c in ">not_a_header") + 3)]
    import gzip
    gz = tmp_path / "g.fa.gz"
    gz.write_bytes(gzip.compress(fa.read_bytes()))
    assert subprocess.run([exe, str(gz)], capture_output=True, text=True).stdout == r.stdout


# ---- the host twin and the stream under AddressSanitizer and UBSan, as a program of its own ----------------------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    """tests/tools/mappings_host_test.cpp: csrc/mappings.hpp and csrc/cli/mappings_stream.hpp under a host compiler alone (they need no HIP), the
    sanitizers' runtimes linked in; it has its own main and runs as it is, nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("san") / "mappings_host_test")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "mappings_host_test.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("geo", sorted(MC.GEOMETRIES))
def test_host_twin_under_sanitizers_equals_the_judge(sanitized_program, geo, tmp_path):
    G = MC.GEOMETRIES[geo]
    good = [MC.records(G, n, mode) for mode in MC.MODES for n in MC.SIZES]
    bad = list(MC.refused().values()) if geo == "nine" else []
    cases = good + [b[0] for b in bad]
    blob = struct.pack("<I", len(G["seq_len"])) + np.asarray(G["seq_len"], "<u8").tobytes() + struct.pack("<IIQ", G["read_len"], G["overlap"], len(cases))
    for c in cases:
        blob += struct.pack("<Q", len(c)) + np.asarray(c, "<u4").tobytes()
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    r = subprocess.run([sanitized_program, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"ok: {len(cases)} cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = re.findall(r"^case (.*)$", r.stdout, re.M)
    assert len(lines) == len(cases)
    names = ["" if s == 2 else "s%d" % s for s in range(len(G["seq_len"]))]
    for c, line in zip(good, lines):
        assert bytes.fromhex(line) == MR.pack(MR.lift(c, **G), G["seq_len"], names, G["read_len"], G["overlap"])
    for (_, first, code), line in zip(bad, lines[len(good):]):
        assert line.startswith("refused record %d: %d " % (first, code))
