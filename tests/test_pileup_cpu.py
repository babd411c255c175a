"""CPU suite of the pileup (`colord_hip compress-* -G genome --pileup`, `info --pileup`).  The judge is tests/pileup_ref.py (numpy,
written from the definition).  Here: the host twin (cl_pileup_host) equals the judge on the constructed cases of tests/pileupcases.py, column for
column, site for site, total for total; it refuses the malformed streams of tests/editstreams.py with the codes and reads of the edit profile; the
ABI; the `hippileup` stream through `info --pileup` as a table, as a VCF and as a summary, and every refusal of its reader; the options; the host
twin and the stream's code under AddressSanitizer and UBSan as a program of its own.  No GPU is needed."""
import ctypes as C
import json
import os
import re
import struct
import subprocess
import numpy as np
import pytest
from colord_amd import _native as N, archive as AR
import editstreams as ES
import pileup_ref as PR
import pileupcases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
GOLDEN_ARC = os.path.join(ROOT, "tests", "golden", "archives", "bovis24_q_4-avg_balanced.colord")


def host_pileup(case, streams, thr=PR.DEFAULTS, refs=None):
    """cl_pileup_host -> (status, (n_pos, 8) columns, (m, 12) sites, totals, bad read, bad code); the need of the sites is asked for first, and a call
    with too little room must report it and leave the sites' buffer as it was"""
    lib = N.load()
    refs = case.refs if refs is None else refs
    rc = np.ascontiguousarray(np.concatenate(refs), dtype=np.uint8)
    roff = np.cumsum([0] + [len(r) for r in refs]).astype(np.uint64)
    raw = np.frombuffer(b"".join(streams), np.uint8).copy() if streams else np.zeros(1, np.uint8)
    off = np.cumsum([0] + [len(s) for s in streams]).astype(np.uint64)
    sl = np.ascontiguousarray(case.seq_len, dtype=np.uint64)
    cols = np.full((int(sl.sum()) + 1, 8), 0xabababab, np.uint32)                         # one row more than the table has: it must stay as it is
    sums, n, bad, code = N.PileupSums(), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    args = (rc.ctypes.data, roff.ctypes.data, len(refs), sl.ctypes.data if len(sl) else None, len(sl), case.read_len, case.overlap, raw.ctypes.data, off.ctypes.data, len(streams), *thr)
    st = lib.cl_pileup_host(*args, None, None, 0, C.byref(n), C.byref(sums), C.byref(bad), C.byref(code))
    if st not in (N.CL_OK, N.CL_E_CAPACITY):
        st2 = lib.cl_pileup_host(*args, cols.ctypes.data, None, 0, C.byref(n), C.byref(sums), C.byref(bad), C.byref(code))
        assert st2 == st and (cols == 0xabababab).all(), "something was written although the call failed"
        return st, None, None, None, bad.value, code.value
    need = n.value
    sites = np.full((need + 1, 12), 0xabababab, np.uint32)
    if need:
        assert lib.cl_pileup_host(*args, None, sites.ctypes.data, need - 1, C.byref(n), C.byref(sums), None, None) == N.CL_E_CAPACITY and n.value == need and (sites == 0xabababab).all()
    st = lib.cl_pileup_host(*args, cols.ctypes.data, sites.ctypes.data, need, C.byref(n), C.byref(sums), C.byref(bad), C.byref(code))
    assert n.value == need and (sites[need] == 0xabababab).all() and (cols[-1] == 0xabababab).all()
    return st, cols[:-1].copy(), sites[:need].copy(), sums.as_dict(), bad.value, code.value


# ---- the host twin against the judge ------------------------------------------------------------------------------------------------------
def test_the_constructed_cases_hold_what_they_say():
    G = PC.groups()
    want = {"insertion_runs_without_a_position": dict(ins=0, ins_unplaced=4), "insertion_runs_at_the_last_base": dict(ins=5, ins_unplaced=0), "reads_on_reads": dict(reads=0, covered=0),
            "insertion_run_over_the_windows_edge": dict(ins=4, ins_unplaced=0), "insertion_run_cut_by_a_change_of_reference": dict(ins=8, ins_unplaced=2),
            "contention_1025_reads_on_one_position": dict(reads=1025, sub=1025, ins=1025, match=3075), "every_substitution": dict(sub=600, covered=100, match=0)}
    for name, t in want.items():
        got = PC.nine(G[name]).judged().totals()
        assert {k: got[k] for k in t} == t, name
    J = PC.nine(G["anchors_at_both_ends_of_the_table"]).judged()
    assert J.cols[0, 0] == 2 and J.cols[PC.N_POS - 1, 0] == 3 and J.diff[PC.N_POS] == -3 and J.diff[0] == 2            # an anchor from position 0, three that end exactly at n_pos
    J = PC.nine(G["same_positions_through_two_pieces"]).judged()
    assert (J.cols[80:95, 0] >= 2).all() and J.cols[85, 1:5].sum() == 1 and J.cols[86, 5] == 1 and J.cols[86, 6] == 1       # both pieces reach 80 .. 94 of sequence 0
    J = PC.nine(G["every_substitution"]).judged()
    o = J.origin[16]
    for x in range(o, o + 100):                                                             # every read base but the genome's own, from both orientations
        assert [int(v) for b, v in enumerate(J.cols[x, 1:5]) if b != J.cols[x, 7]] == [2, 2, 2] and J.cols[x, 1 + J.cols[x, 7]] == 0
    assert set(J.cols[o:o + 100, 7].tolist()) == {0, 1, 2, 3}
    J = PC.nine(G["thresholds"]).judged()
    base = J.origin[10]
    at = lambda thr: {int(s[1]) for s in J.sites(*thr) if s[0] == 5}
    assert at(PR.DEFAULTS) == {20, 30, 50, 60, 75} and at((13, 3, 230)) == {40} and at((13, 3, 231)) == set()
    assert 65 in at((1, 1, 333)) and 65 not in at((1, 1, 334)) and 70 in at((0, 0, 0)) and 70 not in at((1, 0, 0))
    kinds = {int(s[1]): int(s[3]) for s in J.sites() if s[0] == 5}
    ref50 = int(J.cols[base + 50, 7])
    assert kinds[60] == 4 and kinds[75] == 4 and kinds[50] == min(b for b in range(4) if b != ref50 and J.cols[base + 50, 1 + b] == 3)


def test_host_twin_equals_the_judge_on_the_hand_made_streams():
    case, names = PC.hand()
    assert len(case.seq_len) == 69 and len(PR.pieces(case.seq_len, case.read_len, case.overlap)) == 69 and {"anchor70000_at0_rev1", "anchor_len0", "alternatives_64", "anchor63_at1_rev0"} <= set(names)
    J = case.judged()
    for thr in (PR.DEFAULTS, (1, 1, 0), (2, 1, 500)):
        st, cols, sites, sums, _, _ = host_pileup(case, case.streams, thr)
        assert st == N.CL_OK and np.array_equal(cols, J.columns()) and sums == J.totals() and np.array_equal(sites, J.sites(*thr)), thr
    assert J.totals()["reads"] == sum(1 for s in case.streams if s[0] >> 4 == ES.START_ES) - 1 and J.totals()["ins_unplaced"] > 0          # (every script read but `start_only`)
    bad = []
    for name, s in zip(names, case.streams):                                                # one by one, so that a difference names the stream
        Js = case.judged([s])
        st, cols, sites, sums, _, _ = host_pileup(case, [s], (1, 1, 500))
        if st != N.CL_OK or not np.array_equal(cols, Js.columns()) or sums != Js.totals() or not np.array_equal(sites, Js.sites(1, 1, 500)):
            bad.append(name)
    assert not bad, bad[:5]


@pytest.mark.parametrize("name", sorted(PC.groups()) + ["everything"])
def test_host_twin_equals_the_judge_on_the_constructed_groups(name):
    streams = PC.everything() if name == "everything" else PC.groups()[name]
    case = PC.nine(streams)
    J = case.judged()
    for thr in PC.THRESHOLDS:
        st, cols, sites, sums, _, _ = host_pileup(case, streams, thr)
        assert st == N.CL_OK and np.array_equal(cols, J.columns()) and sums == J.totals(), (name, thr)
        assert np.array_equal(sites, J.sites(*thr)), (name, thr)


@pytest.mark.parametrize("n", PC.READ_COUNTS)
def test_read_counts(n):
    pool = PC.everything()
    streams = (pool * (n // len(pool) + 1))[:n]
    case = PC.nine(streams)
    J = case.judged()
    st, cols, sites, sums, _, _ = host_pileup(case, streams, (1, 1, 0))
    assert st == N.CL_OK and np.array_equal(cols, J.columns()) and sums == J.totals() and np.array_equal(sites, J.sites(1, 1, 0))


def test_malformed_streams_give_the_codes_and_reads_of_the_profile():
    from test_edits_cpu import host_profile
    case, _ = PC.hand()
    good = [case.streams[3], case.streams[40], case.streams[41]]
    for name, (bad, why) in {**ES.malformed_host(), **ES.malformed_device()}.items():
        st, cols, _, _, read, code = host_pileup(case, good + [bad] + good)
        pst, _, pread, pwhy = host_profile(good + [bad] + good, case.refs)
        assert st == N.CL_E_INVALID and cols is None and read == 3 == pread and pst == N.CL_E_INVALID, name
        assert N.load().cl_edit_profile_error(code).decode() == why == pwhy, name


def test_geometries_that_are_refused():
    case = PC.nine([])
    g = lambda **kw: type("G", (), {**dict(refs=case.refs, seq_len=case.seq_len, read_len=100, overlap=30), **kw})
    assert host_pileup(g(read_len=30), [])[0] == N.CL_E_INVALID
    assert host_pileup(g(read_len=110), [])[0] == N.CL_E_INVALID                           # pieces of other lengths than the references
    assert host_pileup(g(seq_len=case.seq_len + [500] * 3), [])[0] == N.CL_E_INVALID       # more pieces than references
    st, cols, sites, sums, _, _ = host_pileup(case, [])
    assert st == N.CL_OK and not cols[:, :7].any() and np.array_equal(cols[:, 7], np.concatenate(case.seqs)) and len(sites) == 0 and sums == dict.fromkeys(PR.TOTALS, 0)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
NAMES = ["cl_pileup_create", "cl_pileup_add", "cl_pileup_finish", "cl_pileup_columns", "cl_pileup_sites", "cl_pileup_totals", "cl_pileup_free", "cl_pileup_positions", "cl_pileup_host",
         "cl_ctx_set_pileup", "cl_compressor_pileup"]


def test_abi_names():
    header = open(os.path.join(ROOT, "include", "colord_hip.h")).read()
    lib = N.load()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in N.exported_names() and hasattr(lib, n)
    from colord_amd import device as D
    assert hasattr(D.Context, "set_pileup") and hasattr(D.Context, "pileup") and hasattr(D.Compressor, "pileup")
    for name in ("add", "finish", "columns", "sites", "totals"):
        assert hasattr(D.Pileup, name)
    for n in ("cl_pileup_host", "cl_ctx_set_pileup"):
        assert n in D._OrderedLib._HOST_ONLY
    assert "pileup (DESIGN.md 4n" in header and "are not tuned against anything" in header and C.sizeof(N.PileupSums) == 56


# ---- the stream through `info` -----------------------------------------------------------------------------------------------------------
def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def stamp(path, payload):
    arc = AR.read_archive(GOLDEN_ARC)
    AR.write_archive(path, list(arc.values()) + [AR.Stream("hippileup", 0, [(0, payload)])])


SEQ_NAMES = ["chrA", "empty", "", "chr3", "chr4", "chr5", "one", "chr7", "last|x"]        # (a sequence without a name is printed by its index)
STORED = (1, 1, 0)


@pytest.fixture(scope="module")
def hand_built(tmp_path_factory):
    J = PC.nine(PC.everything()).judged()
    payload = PR.pack(J.sites(*STORED), J.seq_len, SEQ_NAMES, 100, 30, STORED, J.totals())
    arc = str(tmp_path_factory.mktemp("pile") / "p.colord")
    stamp(arc, payload)
    return arc, PR.parse(payload)


def test_pack_and_parse_round_trip(hand_built):
    _, S = hand_built
    J = PC.nine(PC.everything()).judged()
    assert S["seq_len"] == J.seq_len and S["names"] == SEQ_NAMES and S["thresholds"] == STORED and S["totals"] == J.totals() and np.array_equal(S["sites"], J.sites(*STORED))
    assert len(PR.pack(S["sites"], J.seq_len, SEQ_NAMES, 100, 30, STORED, J.totals())) == 96 + sum(10 + len(n) for n in SEQ_NAMES) + 48 * len(S["sites"])
    assert {int(k) for k in S["sites"][:, 3]} == {0, 1, 2, 3, 4, 5} and {int(s) for s in S["sites"][:, 0]} >= {0, 2, 5, 6, 8}


def test_info_prints_the_table_the_vcf_and_the_summary(hand_built, tmp_path):
    arc, S = hand_built
    r = run("info", "--pileup", arc)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == PR.tsv_lines(S["sites"], SEQ_NAMES) and len(r.stdout.splitlines()) == len(S["sites"]) > 100
    rows = [line.split("\t") for line in r.stdout.splitlines()]
    assert all(len(c) == 11 and c[2] in "ACGT" and c[10] in PR.KINDS and c[10] != c[2] for c in rows) and {c[0] for c in rows} >= {"chrA", "2", "last|x"}
    assert all(int(c[3]) == sum(int(v) for v in c[4:9]) for c in rows)                     # depth = A + C + G + T + del: the reference base's column is `match`
    for opts, ma, pm in ((["--min-alt", "3"], 3, 0), (["--min-frac", "0.5"], 0, 500), (["--min-alt", "2", "--min-frac", "0.334"], 2, 334), (["--min-frac", "1"], 0, 1000), (["--min-alt", "0"], 0, 0)):
        r = run("info", "--pileup", *opts, arc)
        assert r.returncode == 0 and r.stdout.splitlines() == PR.tsv_lines(S["sites"], SEQ_NAMES, ma, pm), opts
    a, b = PR.tsv_lines(S["sites"], SEQ_NAMES, 3, 0), PR.tsv_lines(S["sites"], SEQ_NAMES, 2, 334)
    assert 0 < len(a) < len(S["sites"]) and 0 < len(b) < len(S["sites"]) and a != b
    r = run("info", "--pileup", "--vcf", arc)
    assert r.returncode == 0 and r.stdout.splitlines() == PR.vcf_lines(S["sites"], S["seq_len"], SEQ_NAMES)
    body = [line.split("\t") for line in r.stdout.splitlines() if not line.startswith("#")]
    assert r.stdout.startswith("##fileformat=VCFv4.2\n") and len(body) == int((S["sites"][:, 3] < 4).sum()) > 0 and all(len(c) == 8 and len(c[3]) == 1 and len(c[4]) == 1 and c[3] != c[4] for c in body)
    assert all(re.fullmatch(r"DP=\d+;AD=\d+,\d+;AF=\d\.\d{4}", c[7]) for c in body) and "##contig=<ID=2,length=70>" in r.stdout
    r = run("info", "--pileup", "--vcf", "--min-alt", "3", arc)
    assert r.returncode == 0 and r.stdout.splitlines() == PR.vcf_lines(S["sites"], S["seq_len"], SEQ_NAMES, 3, 0)
    r = run("info", "--pileup", "--summary", "--json", arc)
    assert r.returncode == 0 and json.loads(r.stdout) == PR.summary(S)
    s = json.loads(r.stdout)
    assert s["positions"] == PC.N_POS and s["sites"] == len(S["sites"]) == sum(s["sites_by_kind"].values()) and s["mean_depth"] > 1 and 0 < s["sub_rate"] < 1 and s["ins_unplaced"] == 6
    r = run("info", "--pileup", "--summary", arc)
    assert r.returncode == 0 and "positions: %d" % PC.N_POS in r.stdout and "sites (depth >= 1, alternative >= 1 columns and >= 0 permille of the depth): %d" % len(S["sites"]) in r.stdout
    dec = str(tmp_path / "d.fastq")
    assert run("decompress", arc, dec).returncode == 0                                  # `decompress` ignores the stream ...
    assert run("decompress", GOLDEN_ARC, str(tmp_path / "o.fastq")).returncode == 0
    assert open(dec).read() == open(str(tmp_path / "o.fastq")).read()
    assert run("check", arc).returncode == 0                                            # ... and so does `check`
    i = run("info", arc)
    assert i.returncode == 0 and "pileup: %d sites on the 9 sequences" % len(S["sites"]) in i.stderr
    plain = run("info", GOLDEN_ARC)
    assert plain.returncode == 0 and "pileup" not in plain.stderr
    none = run("info", "--pileup", GOLDEN_ARC)
    assert none.returncode == 1 and "no pileup is stored" in none.stderr
    empty = str(tmp_path / "e.colord")
    stamp(empty, PR.pack(np.zeros((0, 12), np.uint32), S["seq_len"], SEQ_NAMES, 100, 30, PR.DEFAULTS, dict.fromkeys(PR.TOTALS, 0)))
    r = run("info", "--pileup", empty)
    assert r.returncode == 0 and r.stdout == ""
    r = run("info", "--pileup", "--summary", "--json", empty)
    assert r.returncode == 0 and json.loads(r.stdout)["mean_depth"] == 0 and json.loads(r.stdout)["sites"] == 0


def bad_payloads():
    J = PC.nine(PC.groups()["thresholds"]).judged()
    sites, sl, t = J.sites(), J.seq_len, J.totals()
    assert len(sites) == 5
    pk = lambda s, **kw: PR.pack(s, sl, SEQ_NAMES, 100, 30, PR.DEFAULTS, t, **kw)
    good = pk(sites)
    table_end = len(good) - 48 * len(sites)

    def changed(row, col, v):
        s = sites.copy(); s[row, col] = v
        return pk(s)
    long_name = bytearray(good); struct.pack_into("<H", long_name, 96 + 8, 60000)
    return {"version_2": pk(sites, version=2), "record_size_44": pk(sites, record_bytes=44), "one_byte_short": good[:-1], "one_site_short": good[:-48], "count_one_more": pk(sites, count=6),
            "head_cut": good[:90], "name_table_cut": good[:table_end - 3], "name_longer_than_the_stream": bytes(long_name), "one_sequence_more": good[:8] + struct.pack("<I", 10) + good[12:],
            "sequences_without_bytes": good[:8] + struct.pack("<I", 0xffffffff) + good[12:], "sequence_outside_the_table": changed(4, 0, 9), "position_at_the_sequences_end": changed(2, 1, sl[5]),
            "position_on_an_empty_sequence": changed(0, 0, 1), "reference_base_4": changed(1, 2, 4), "kind_6": changed(1, 3, 6), "kind_is_the_reference_base": changed(1, 3, int(sites[1, 2])),
            "sites_out_of_order": pk(sites[[0, 2, 1, 3, 4]]), "a_site_twice": pk(sites[[0, 1, 1, 2, 3]])}


@pytest.mark.parametrize("how", sorted(bad_payloads()))
def test_a_stream_of_another_shape_is_refused_cleanly(how, tmp_path):
    payload = bad_payloads()[how]
    with pytest.raises(ValueError):
        PR.parse(payload)
    arc = str(tmp_path / "s.colord")
    stamp(arc, payload)
    for mode in ([], ["--vcf"], ["--summary"], ["--summary", "--json"]):
        r = run("info", "--pileup", *mode, arc)
        assert r.returncode == 1 and "`hippileup` stream is not one this build reads" in r.stderr and r.stdout == ""
    i = run("info", arc)
    assert i.returncode == 0 and "a `hippileup` stream this build cannot read" in i.stderr


def test_help_and_refused_combinations(tmp_path):
    r = run("compress-ont", "--help")
    assert r.returncode == 0 and "--pileup" in r.stderr and "hippileup" in r.stderr and "THE FULL TABLE IS NOT STORED" in r.stderr and "NOT TUNED AGAINST ANYTHING" in r.stderr
    assert "info --pileup [--min-alt N] [--min-frac F] [--vcf] | --pileup --summary [--json] archive.colord" in r.stderr
    out = str(tmp_path / "out.colord")
    for extra, text in (([], "--pileup needs a reference genome (-G)"), (["-G", "genome.fa", "--gpus", "2"], "--pileup is not available with --gpus > 1"),
                        (["-G", "genome.fa", "--domains", "2"], "--pileup is not available with --domains > 1"), (["-G", "genome.fa", "--overlaps"], "--pileup is not available with --overlaps"),
                        (["-G", "genome.fa", "--pileup-min-frac", "1.5"], "--pileup-min-frac must be in [0, 1]"), (["-G", "genome.fa", "--pileup-min-frac", "x"], "--pileup-min-frac must be in [0, 1]"),
                        (["-G", "genome.fa", "--pileup-min-depth", "-1"], "--pileup-min-depth must be in"), (["-G", "genome.fa", "--pileup-min-alt", "-2"], "--pileup-min-alt must be in")):
        r = run("compress-ont", "--pileup", *extra, "in.fq", out)
        assert r.returncode == 1 and text in r.stderr and not os.path.exists(out), r.stderr
    for opt in (["--pileup-min-depth", "3"], ["--pileup-min-alt", "3"], ["--pileup-min-frac", "0.5"]):
        r = run("compress-ont", "-G", "genome.fa", *opt, "in.fq", out)
        assert r.returncode == 1 and "need --pileup" in r.stderr and not os.path.exists(out)
    for args in (["--vcf"], ["--min-alt", "2"], ["--min-frac", "0.5"], ["--pileup", "--summary", "--vcf"], ["--pileup", "--summary", "--min-alt", "2"], ["--pileup", "--json"], ["--pileup", "--vcf", "--json"],
                 ["--pileup", "--mappings"], ["--pileup", "--overlaps"], ["--pileup", "--report"], ["--pileup", "--coverage", "10"], ["--pileup", "--names"], ["--mappings", "--vcf"], ["--summary"]):
        r = run("info", *args, GOLDEN_ARC)
        assert r.returncode == 1 and "usage" in r.stderr and "--pileup" in r.stderr, args
    for args, text in ((["--pileup", "--min-alt", "x"], "--min-alt needs a number"), (["--pileup", "--min-alt"], "--min-alt needs a number"), (["--pileup", "--min-frac", "2"], "--min-frac needs a fraction"),
                       (["--pileup", "--min-frac", "0.5x"], "--min-frac needs a fraction"), (["--pileup", "--min-frac"], "--min-frac needs a fraction")):
        r = run("info", *args, GOLDEN_ARC)
        assert r.returncode == 1 and text in r.stderr, args


# ---- the host twin and the stream under AddressSanitizer and UBSan, as a program of its own ----------------------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    """tests/tools/pileup_host_test.cpp: csrc/pileup.hpp and csrc/cli/pileup_stream.hpp under a host compiler alone (they need no HIP), the sanitizers'
    runtimes linked in; it has its own main and runs as it is, nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("san") / "pileup_host_test")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "pileup_host_test.cpp"), "-o", exe])
    return exe


def blob_of(case, thr, cases):
    refs = case.refs
    roff = np.cumsum([0] + [len(r) for r in refs]).astype("<u8")
    blob = struct.pack("<I", len(case.seq_len)) + np.asarray(case.seq_len, "<u8").tobytes() + struct.pack("<5I", case.read_len, case.overlap, *thr) + struct.pack("<I", len(refs)) + roff.tobytes()
    blob += np.concatenate(refs).astype(np.uint8).tobytes() + struct.pack("<Q", len(cases))
    for streams in cases:
        blob += struct.pack("<Q", len(streams)) + np.cumsum([0] + [len(s) for s in streams]).astype("<u8").tobytes() + b"".join(streams)
    return blob


@pytest.mark.parametrize("which", ["nine", "hand"])
def test_host_twin_under_sanitizers_equals_the_judge(sanitized_program, which, tmp_path):
    thr = (1, 1, 0)
    if which == "nine":
        case = PC.nine([])
        good = list(PC.groups().values()) + [PC.everything(), []]
        names = ["" if s == 2 else "s%d" % s for s in range(9)]
    else:
        case, _ = PC.hand()
        good = [case.streams]
        names = ["" if s == 2 else "s%d" % s for s in range(69)]
    bad = [[case.streams[0] if which == "hand" else PC.everything()[0], m[0]] for m in {**ES.malformed_host(), **ES.malformed_device()}.values()] if which == "hand" else []
    path = tmp_path / "cases.bin"
    path.write_bytes(blob_of(case, thr, good + bad))
    r = subprocess.run([sanitized_program, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"ok: {len(good) + len(bad)} cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = re.findall(r"^case (.*)$", r.stdout, re.M)
    assert len(lines) == len(good) + len(bad)
    for streams, line in zip(good, lines):
        J = case.judged(streams)
        cols, packed = line.split(" ")
        assert bytes.fromhex(cols) == J.columns().astype(">u4").tobytes()
        assert bytes.fromhex(packed) == PR.pack(J.sites(*thr), case.seq_len, names, case.read_len, case.overlap, thr, J.totals())
    for line in lines[len(good):]:
        assert line.startswith("refused read 1: ")
