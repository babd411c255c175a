"""CPU suite of the overlap records (cl_overlap, `colord_hip compress-* --overlaps`, `info --overlaps`).  The judge is
tests/overlaps_ref.py (plain Python, written from the definition).  Here: the host form of the C ABI equals the judge on the hand-made streams of
tests/editstreams.py and tests/overlapstreams.py and on the reference's own tuple streams (golden es.bin); the invariants of the records on all of
them; malformed streams are refused with nothing written; the ABI; the `hipoverlaps` stream through `info --overlaps`; the host form under
AddressSanitizer and UBSan as a program of its own.  No GPU is needed."""
import ctypes as C
import os
import re
import struct
import subprocess
import numpy as np
import pytest
from colord_amd import _native as N, archive as AR
from util import golden
import edits_ref as E
import editstreams as ES
import overlaps_ref as OR
import overlapstreams as OS
from test_edits_cpu import golden_refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
ARC = os.path.join(ROOT, "tests", "golden", "archives")
GOLDENS = ["c1_ont_default", "c2_hifi_org", "s3m_ont_n_ratio"]


def host_overlaps(streams, refs, first_read=0, ref_read=None, cap=None):
    """cl_overlaps_host -> (status, (n, 12) uint32 records, n_out, bad read, text of the bad code); cap None: the need is asked for first"""
    lib = N.load()
    rc = np.ascontiguousarray(np.concatenate(refs) if refs else np.zeros(0, np.uint8), dtype=np.uint8)
    roff = np.cumsum([0] + [len(r) for r in refs]).astype(np.uint64)
    raw = np.frombuffer(b"".join(streams), np.uint8).copy() if streams else np.zeros(0, np.uint8)
    off = np.cumsum([0] + [len(s) for s in streams]).astype(np.uint64)
    tab = None if ref_read is None else np.ascontiguousarray(ref_read, dtype=np.uint32)
    bad, code, n = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    args = (rc.ctypes.data, roff.ctypes.data, len(refs), raw.ctypes.data, off.ctypes.data, len(streams), first_read, None if tab is None else tab.ctypes.data, 0 if tab is None else len(tab))
    if cap is None:
        st = lib.cl_overlaps_host(*args, None, 0, C.byref(n), C.byref(bad), C.byref(code))
        if st not in (N.CL_OK, N.CL_E_CAPACITY):
            return st, np.zeros((0, 12), np.uint32), n.value, bad.value, lib.cl_edit_profile_error(code.value).decode()
        cap = n.value
    out = np.full((cap + 1, 12), 0xabababab, np.uint32)       # one record more than asked for: it must stay as it is
    st = lib.cl_overlaps_host(*args, out.ctypes.data, cap, C.byref(n), C.byref(bad), C.byref(code))
    assert (out[cap] == 0xabababab).all()
    if st != N.CL_OK:
        assert (out == 0xabababab).all(), "something was written although the call failed"
    return st, out[:n.value if st == N.CL_OK else 0].copy(), n.value, bad.value, lib.cl_edit_profile_error(code.value).decode()


@pytest.fixture(scope="module")
def hand():
    refs = ES.references()
    S = {**ES.hand_made(), **OS.hand_made()}
    names, streams = list(S), list(S.values())
    per = [OR.records_of_read(s, refs)[0] for s in streams]
    return refs, names, streams, per


_judged = {}


def judged(cfg):
    """overlaps_ref over a golden's es.bin with an identity-plus-5 translation table, computed once: (streams, refs, table, records)"""
    if cfg not in _judged:
        streams, refs = [e[2] for e in golden(cfg).es], golden_refs(cfg)
        table = np.arange(len(refs), dtype=np.uint32) + 5
        _judged[cfg] = (streams, refs, table, OR.records(streams, refs, 3, table))
    return _judged[cfg]


# ---- the host form against the reference -------------------------------------------------------------------------------------------------
def test_host_form_equals_the_reference_on_hand_made_streams(hand):
    refs, names, streams, per = hand
    bad = []
    for i, (name, s, want) in enumerate(zip(names, streams, per)):
        st, got, n, _, _ = host_overlaps([s], refs, first_read=i)
        want = np.array([(i,) + w[1:] for w in want], np.uint32).reshape(-1, 12)
        if st != 0 or n != len(want) or not np.array_equal(got, want) or OR.invariants(got):
            bad.append((name, st, got.tolist(), want.tolist()))
    assert not bad, bad[:3]
    table = np.arange(len(refs), dtype=np.uint32)[::-1].copy()
    for sset in (streams, OS.read_set(), OS.read_set() + streams):
        want = OR.records(sset, refs, 11, table)
        st, got, n, _, _ = host_overlaps(sset, refs, 11, table)
        assert st == 0 and n == len(want) and np.array_equal(got, want)
        assert OR.invariants(got) == []
    assert len(OR.records(OS.read_set(), refs)) == 12 * 67


def test_hand_made_streams_cover_the_record(hand):
    """between them the streams exercise every field and both flags (a judge and a host form that agree on nothing show nothing)"""
    _, _, _, per = hand
    recs = np.array([r for p in per for r in p], np.uint32)
    f = {k: recs[:, i] for i, k in enumerate(OR.FIELDS)}
    assert set(f["flags"].tolist()) == {0, 1, 2, 3} and f["subst"].any() and f["anchor_bases"].any() and (f["te"] == f["tlen"]).any() and (f["ts"] == 0).any()
    assert (f["qe"] == f["qlen"]).any() and (f["qe"] < f["qlen"]).any() and (f["qs"] > 0).any() and sum(1 for p in per if not p) >= 8 and max(len(p) for p in per) >= 65


@pytest.mark.parametrize("cfg", GOLDENS)
def test_host_form_equals_the_reference_on_the_goldens(cfg):
    streams, refs, table, want = judged(cfg)
    st, got, n, _, _ = host_overlaps(streams, refs, 3, table)
    assert st == 0 and n == len(want) and np.array_equal(got, want)
    assert OR.invariants(got) == []
    assert len(want) >= sum(1 for s in streams if s[0] >> 4 == E.START_ES)                # (the reference codes no read by script without an aligned column)
    cut = len(streams) // 3                                                              # two calls give the same records as one
    _, a, _, _, _ = host_overlaps(streams[:cut], refs, 3, table)
    _, b, _, _, _ = host_overlaps(streams[cut:], refs, 3 + cut, table)
    assert np.array_equal(np.concatenate([a, b]), want)
    if len(want):                                                                        # the capacity protocol: the need, nothing written
        st, none, n, _, _ = host_overlaps(streams, refs, 3, table, cap=len(want) - 1)
        assert st == N.CL_E_CAPACITY and n == len(want) and len(none) == 0


def test_records_add_up_to_the_profile():
    """the sums over a golden's records against the profile's counters of the same streams (tests/edits_ref.py): two judges, one walk"""
    assert sum(len(judged(cfg)[3]) for cfg in GOLDENS) > 385                            # (c1 is plain reads only; s3m has 385 script reads)
    for cfg in GOLDENS:
        streams, refs, _, want = judged(cfg)
        prof = E.profile(streams, refs)
        assert int(want[:, 10].sum()) == prof["anchor_bases"] and int(want[:, 9].sum()) == int(prof["tuples"][E.SUBST])
        assert int(want[:, 8].sum()) == int(prof["tuples"][E.MATCH]) + prof["anchor_bases"]


# ---- malformed streams -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ES.malformed_host()) + sorted(ES.malformed_device()))
def test_malformed_stream_is_refused_and_nothing_is_written(name, hand):
    refs, _, streams, _ = hand
    bad, why = {**ES.malformed_host(), **ES.malformed_device()}[name]
    with pytest.raises(OR.Malformed) as x:
        OR.records_of_read(bad, refs)
    assert x.value.why == why
    good = [streams[3], streams[40], streams[-2]]
    st, _, n, read, text = host_overlaps(good[:2] + [bad] + good[2:], refs)
    assert st == N.CL_E_INVALID and n == 0 and read == 2 and text == why
    st, _, n, read, text = host_overlaps(good[:2] + [bad] + good[2:], refs, cap=1000)      # with room for everything: still nothing written
    assert st == N.CL_E_INVALID and n == 0 and read == 2 and text == why


def test_an_id_past_the_translation_table_is_refused(hand):
    refs, names, streams, _ = hand
    s = streams[names.index("two_alternatives")]                                       # names the references 0, 1 and 2
    assert host_overlaps([s], refs, 0, np.arange(3, dtype=np.uint32))[0] == 0
    only_0 = streams[names.index("start_and_one_insertion")]
    for size in (2, 1):
        st, _, n, read, text = host_overlaps([only_0, s], refs, 0, np.arange(size, dtype=np.uint32))
        assert st == N.CL_E_INVALID and n == 0 and text == "reference id outside the reference arena" and read == 1
        with pytest.raises(OR.Malformed) as x:
            OR.records([only_0, s], refs, 0, np.arange(size))
        assert x.value.read == 1
    st, got, n, _, _ = host_overlaps([only_0, s], refs, 0, None)                           # (no table at all: the ids as they are)
    assert st == 0 and np.array_equal(got, OR.records([only_0, s], refs)) and set(got[:, 1].tolist()) == {0, 1, 2}


# ---- ABI and the stream ------------------------------------------------------------------------------------------------------------------
NAMES = ["cl_overlaps_of", "cl_overlaps_host", "cl_ctx_set_overlaps", "cl_ctx_overlaps", "cl_compressor_overlaps"]


def test_abi_names_and_sizes():
    header = open(os.path.join(ROOT, "include", "colord_hip.h")).read()
    lib = N.load()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in N.exported_names() and hasattr(lib, n)
    from colord_amd import device as D
    for name in ("set_overlaps", "overlaps", "overlaps_of"):
        assert hasattr(D.Context, name)
    assert hasattr(D.Compressor, "overlaps")
    for n in ("cl_overlaps_host", "cl_ctx_set_overlaps", "cl_ctx_overlaps", "cl_compressor_overlaps"):
        assert n in D._OrderedLib._HOST_ONLY
    assert C.sizeof(N.Overlap) == 48 == OR.RECORD_BYTES
    m = re.search(r"typedef struct cl_overlap \{(.*?)\} cl_overlap;", header, re.S)
    assert tuple(re.findall(r"(\w+)\s*[,;]", m.group(1))) == OR.FIELDS == tuple(k for k, _ in N.Overlap._fields_)
    assert "ERRORS OF THEIR OWN" in header and "REFERENCE reads only" in header


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def stamp(path, payload):
    arc = AR.read_archive(os.path.join(ARC, "bovis24_q_4-avg_balanced.colord"))
    AR.write_archive(path, list(arc.values()) + [AR.Stream("hipoverlaps", 0, [(0, payload)])])


def test_hipoverlaps_round_trip_through_info(tmp_path):
    """records over the reads of a golden archive (24 reads), so that --names finds every id"""
    rng = np.random.default_rng(3)
    recs = []
    for q in range(2, 24):
        for _ in range(int(rng.integers(0, 4))):
            qs, ts = int(rng.integers(0, 500)), int(rng.integers(0, 500))
            m, sb, extra_q, extra_t = int(rng.integers(1, 400)), int(rng.integers(0, 30)), int(rng.integers(0, 20)), int(rng.integers(0, 20))
            recs.append((q, int(rng.integers(0, q)), qs + m + sb + extra_q + 9, ts + m + sb + extra_t + 4, qs, qs + m + sb + extra_q, ts, ts + m + sb + extra_t, m, sb, int(rng.integers(0, m + 1)), int(rng.integers(0, 4))))
    recs = np.array(recs, np.uint32)
    assert OR.invariants(recs) == [] or all(k == "ascending" for _, k in OR.invariants(recs))
    payload = OR.pack_hipoverlaps(recs)
    assert len(payload) == 16 + 48 * len(recs)
    arc = str(tmp_path / "s.colord")
    stamp(arc, payload)
    r = run("info", "--overlaps", arc)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == OR.paf_lines(recs)
    assert all(len(line.split("\t")) == 15 and line.split("\t")[11] == "255" for line in r.stdout.splitlines())
    blocks = sorted(OR.block(x) for x in recs)
    mid = blocks[len(blocks) // 2]
    r = run("info", "--overlaps", "--min-block", str(mid), arc)
    assert r.returncode == 0 and r.stdout.splitlines() == OR.paf_lines(recs, min_block=mid) and 0 < len(r.stdout.splitlines()) < len(recs)
    dec = str(tmp_path / "d.fastq")
    assert run("decompress", arc, dec).returncode == 0                                  # `decompress` ignores the stream ...
    ids = [line[1:].split()[0] for line in open(dec).read().splitlines()[0::4]]
    assert run("decompress", os.path.join(ARC, "bovis24_q_4-avg_balanced.colord"), str(tmp_path / "o.fastq")).returncode == 0
    assert open(dec).read() == open(str(tmp_path / "o.fastq")).read() and len(ids) == 24
    r = run("info", "--overlaps", "--names", arc)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == OR.paf_lines(recs, names=ids)
    assert run("check", arc).returncode == 0                                            # ... and so does `check`
    i = run("info", arc)
    assert i.returncode == 0 and "overlaps: %d records" % len(recs) in i.stderr
    plain = run("info", os.path.join(ARC, "bovis24_q_4-avg_balanced.colord"))
    assert plain.returncode == 0 and "overlaps" not in plain.stderr
    none = run("info", "--overlaps", os.path.join(ARC, "bovis24_q_4-avg_balanced.colord"))
    assert none.returncode == 1 and "no overlaps are stored" in none.stderr
    empty = str(tmp_path / "e.colord")
    stamp(empty, OR.pack_hipoverlaps(np.zeros((0, 12), np.uint32)))
    r = run("info", "--overlaps", empty)
    assert r.returncode == 0 and r.stdout == ""
    stamp(empty, OR.pack_hipoverlaps(np.array([[30, 1, 9, 9, 0, 5, 0, 5, 5, 0, 0, 0]], np.uint32)))      # read 30 of 24
    r = run("info", "--overlaps", "--names", empty)
    assert r.returncode == 1 and "names a read" in r.stderr


@pytest.mark.parametrize("how", ["version_2", "record_size_44", "one_byte_short", "one_record_short", "count_one_more", "header_cut"])
def test_a_stream_of_another_shape_is_refused_cleanly(how, tmp_path):
    good = OR.pack_hipoverlaps(np.arange(36, dtype=np.uint32).reshape(3, 12))
    payload = {"version_2": struct.pack("<I", 2) + good[4:], "record_size_44": good[:4] + struct.pack("<I", 44) + good[8:], "one_byte_short": good[:-1], "one_record_short": good[:-48],
               "count_one_more": good[:8] + struct.pack("<Q", 4) + good[16:], "header_cut": good[:12]}[how]
    arc = str(tmp_path / "s.colord")
    stamp(arc, payload)
    r = run("info", "--overlaps", arc)
    assert r.returncode == 1 and "`hipoverlaps` stream is not one this build reads" in r.stderr and r.stdout == ""
    i = run("info", arc)
    assert i.returncode == 0 and "a `hipoverlaps` stream this build cannot read" in i.stderr


def test_help_and_refused_combinations(tmp_path):
    r = run("compress-ont", "--help")
    assert r.returncode == 0 and "--overlaps" in r.stderr and "hipoverlaps" in r.stderr and "ERRORS OF" in r.stderr and "REFERENCE READS ONLY" in r.stderr
    assert "info --overlaps [--min-block N] [--names] archive.colord" in r.stderr
    r = run("compress-ont", "--overlaps", "in.fq")
    assert r.returncode == 1 and "expected input and output paths" in r.stderr and "unknown option" not in r.stderr
    for extra, text in ((["--gpus", "2"], "--overlaps is not available with --gpus > 1"), (["--domains", "2"], "--overlaps is not available with --domains > 1"),
                        (["-G", "genome.fa"], "--overlaps is not available with -G")):
        r = run("compress-ont", "--overlaps", *extra, "in.fq", str(tmp_path / "out.colord"))
        assert r.returncode == 1 and text in r.stderr, r.stderr
    for args in (["--names"], ["--min-block", "5"], ["--overlaps", "--report"], ["--overlaps", "--json"]):
        r = run("info", *args, os.path.join(ARC, "bovis24_q_4-avg_balanced.colord"))
        assert r.returncode == 1 and "usage" in r.stderr


# ---- the host form under AddressSanitizer and UBSan, as a program of its own ------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    """tests/tools/overlaps_host_test.cpp: csrc/overlaps.hpp and csrc/cli/overlaps_stream.hpp under a host compiler alone (they need no HIP), the
    sanitizers' runtimes linked in; it has its own main and runs as it is, nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("san") / "overlaps_host_test")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "overlaps_host_test.cpp"), "-o", exe])
    return exe


def test_host_form_under_sanitizers_equals_the_reference(sanitized_program, hand, tmp_path):
    refs, _, streams, _ = hand
    bad = {**ES.malformed_host(), **ES.malformed_device()}
    sets = [streams, OS.read_set()]
    cases = [[s] for s in streams] + sets + [[streams[0], b, streams[1]] for b, _ in bad.values()]
    blob = struct.pack("<I", len(refs)) + np.cumsum([0] + [len(r) for r in refs]).astype("<u8").tobytes() + b"".join(r.tobytes() for r in refs) + struct.pack("<Q", len(cases))
    for c in cases:
        blob += struct.pack("<Q", len(c)) + np.cumsum([0] + [len(s) for s in c]).astype("<u8").tobytes() + b"".join(c)
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    r = subprocess.run([sanitized_program, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"ok: {len(cases)} cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = re.findall(r"^case (.*)$", r.stdout, re.M)
    assert len(lines) == len(cases)
    table = np.arange(len(refs), dtype=np.uint32) + 1000                              # the program's: id -> 1000 + id, first read 7
    for c, line in zip(cases[:len(streams) + len(sets)], lines):
        assert bytes.fromhex(line) == OR.pack_hipoverlaps(OR.records(c, refs, 7, table))
    for (_, why), line in zip(bad.values(), lines[len(streams) + len(sets):]):
        assert line == "refused read 1: " + why
