"""CPU suite of the edit-operation profile (cl_edits, `colord_hip compress-* --edit-profile`, `info --edit-profile`).  The judge is
tests/edits_ref.py (plain Python, written from the format table and the definitions).  Here: the reference's own tuple streams (golden
es.bin) satisfy the invariants through the judge; the host form of the C ABI equals the judge on them and on the hand-made streams of
tests/editstreams.py; malformed streams are refused with nothing added; the ABI; the `hipedits` stream through `info`; the host form under
AddressSanitizer and UBSan as a program of its own.  No GPU is needed."""
import ctypes as C
import gzip
import json
import os
import re
import struct
import subprocess
import numpy as np
import pytest
from colord_amd import _native as N, archive as AR
from util import ALL_CONFIGS, GOLD, DATA, golden
import edits_ref as E
import editstreams as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
ARC = os.path.join(ROOT, "tests", "golden", "archives")
WITH_ES = [c for c in ALL_CONFIGS if os.path.exists(os.path.join(GOLD, c, "es.bin.gz"))]


def genome_pseudo_reads(g):
    """the pseudo reads of a -G golden: reference reads 0 .. n_pseudo - 1 (20 x the mean read length, overlap (k - 1) * 10; only A, C, G, T of the genome kept)"""
    lut = np.full(256, 255, np.uint8)
    for ch, v in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
        lut[ch] = v
    seqs, cur = [], []
    for line in gzip.open(os.path.join(DATA, g.spec["genome"] + ".gz"), "rb"):
        if line.startswith(b">"):
            if cur:
                seqs.append(np.concatenate(cur))
            cur = []
        else:
            v = lut[np.frombuffer(line.strip(), np.uint8)]
            cur.append(v[v < 4])
    if cur:
        seqs.append(np.concatenate(cur))
    read_len, overlap, out = 20 * g.p("mean_read_len"), (g.p("k") - 1) * 10, []
    for s in seqs:
        for start in range(0, len(s), read_len - overlap):
            out.append(s[start:min(start + read_len, len(s))])
    assert len(out) == g.p("n_pseudo")
    return out


def golden_refs(cfg):
    """the reference reads a golden's tuple streams point to: the accepted reads free of N, in input order (ref_subset of tests/test_gpu_dna.py),
    behind the pseudo reads of a reference genome"""
    g = golden(cfg)
    rs = g.reads
    ok = g.accept[len(g.accept) - rs.n_reads:].astype(bool) & ~rs.has_n()             # (with a genome the acceptor saw the pseudo reads first)
    refs = [rs.read(i) for i in np.nonzero(ok)[0]]
    return (genome_pseudo_reads(g) if g.spec.get("genome") else []) + refs


_judged = {}


def judged(cfg):
    """edits_ref over a golden's es.bin, computed once"""
    if cfg not in _judged:
        _judged[cfg] = E.profile([e[2] for e in golden(cfg).es], golden_refs(cfg))
    return _judged[cfg]


def new_edits():
    e = N.Edits()
    N.load().cl_edits_clear(C.byref(e))
    return e


def host_profile(streams, refs, acc=None):
    """cl_edit_profile_host -> (status, Edits, bad read, text of the bad code)"""
    lib = N.load()
    acc = new_edits() if acc is None else acc
    rc = np.ascontiguousarray(np.concatenate(refs) if refs else np.zeros(0, np.uint8), dtype=np.uint8)
    roff = np.cumsum([0] + [len(r) for r in refs]).astype(np.uint64)
    raw = np.frombuffer(b"".join(streams), np.uint8).copy() if streams else np.zeros(0, np.uint8)
    raw = np.concatenate([raw, np.zeros(0, np.uint8)])
    off = np.cumsum([0] + [len(s) for s in streams]).astype(np.uint64)
    bad, code = C.c_uint64(0), C.c_uint32(0)
    st = lib.cl_edit_profile_host(rc.ctypes.data, roff.ctypes.data, len(refs), raw.ctypes.data, off.ctypes.data, len(streams), C.byref(acc), C.byref(bad), C.byref(code))
    return st, acc, bad.value, lib.cl_edit_profile_error(code.value).decode()


# ---- 1. + 2. the reference's own streams ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", WITH_ES)
def test_reference_streams_satisfy_the_invariants(cfg):
    want = judged(cfg)
    rs = golden(cfg).reads
    assert E.invariants(want) == []
    assert want["reads"] == rs.n_reads and want["bases"] == len(rs.bases)
    assert int(want["kind_bytes"].sum()) == sum(len(e[2]) for e in golden(cfg).es)


@pytest.mark.parametrize("cfg", WITH_ES)
def test_host_form_equals_the_reference_on_the_goldens(cfg):
    streams = [e[2] for e in golden(cfg).es]
    refs = golden_refs(cfg)
    st, got, _, _ = host_profile(streams, refs)
    assert st == 0
    assert E.same(got.as_dict(), judged(cfg)) is None, E.same(got.as_dict(), judged(cfg))
    assert E.invariants(got.as_dict()) == []
    cut = len(streams) // 3                                                     # two calls into one total, and two totals added
    _, acc, _, _ = host_profile(streams[:cut], refs)
    st, acc, _, _ = host_profile(streams[cut:], refs, acc)
    assert st == 0 and E.same(acc.as_dict(), judged(cfg)) is None
    _, a, _, _ = host_profile(streams[:cut], refs)
    _, b, _, _ = host_profile(streams[cut:], refs)
    N.load().cl_edits_add(C.byref(a), C.byref(b))
    assert E.same(a.as_dict(), judged(cfg)) is None


def test_goldens_cover_the_fields():
    """between them the goldens exercise every kind of field (a judge and a host form that agree on zeros show nothing)"""
    tot = E.empty()
    for cfg in WITH_ES:
        tot = E.add(tot, judged(cfg))
    assert all(int(x) for x in tot["tuples"]) and tot["kind_reads"].all() and tot["main_rev"].all()
    assert tot["skip_entries"] and tot["skip_bases"] and tot["alt_hist"][1:].any() and np.count_nonzero(tot["sub"]) == 12
    assert tot["ins_run_hist"][2:].any() and tot["del_run_hist"][2:].any() and tot["identity_hist"].any()


# ---- hand-made streams ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    refs = ES.references()
    S = ES.hand_made()
    names, streams = list(S), list(S.values())
    per = [E.profile_of_read(s, refs, i) for i, s in enumerate(streams)]      # (raises if a stream leaves its references)
    return refs, names, streams, per


def test_hand_made_streams_say_what_they_were_made_for(hand):
    _, names, _, per = hand
    p = lambda n: per[names.index(n)]
    assert p("alt_id_ends_the_window_skip_starts_the_next")["skip_entries"] == 1 and p("alt_id_ends_the_window_skip_starts_the_next")["skip_entry_sum"] == 11
    assert p("alt_id_ends_the_window_skip_starts_the_next")["skip_bases"] == 0
    assert p("skip_after_main_ref")["skip_entries"] == 1 and p("skip_after_main_ref")["skip_bases"] == 4 and p("skip_first")["skip_bases"] == 5 and p("skip_first")["skip_entries"] == 0
    assert p("alt_id_without_skip")["skip_entries"] == 0 and p("alt_id_without_skip")["skip_bases"] == 6
    for L in (15, 16, 17, 200):
        assert p(f"ins_run{L}")["ins_run_hist"][min(L, 16)] == 1 and p(f"ins_run{L}")["ins_run_hist"].sum() == 1 and p(f"del_run{L}")["del_run_hist"][min(L, 16)] == 1
    for L in (2, 3, 4):
        for first in range(1, L):
            assert p(f"ins_run{L}_split{first}")["ins_run_hist"][L] == 1 and p(f"del_run{L}_split{first}")["del_run_hist"][L] == 1
    assert p("ins_run_then_del_run")["ins_run_hist"][3] == 1 and p("ins_run_then_del_run")["del_run_hist"][2] == 1
    assert p("del_run_over_the_edge_then_ins_run")["del_run_hist"][4] == 1 and p("del_run_over_the_edge_then_ins_run")["ins_run_hist"][16] == 1
    for a, b in ((1, 1), (2, 2), (31, 5), (32, 6), (63, 6), (64, 7), (4095, 12), (4096, 13), (70_000, 17)):
        assert p(f"anchor_len{a}")["anchor_len_hist"][b] == 1 and p(f"skip_len{a}")["skip_len_hist"][b] == 1
    assert p("anchor_len0")["anchor_len_hist"][0] == 1 and p("anchor_len0")["skip_len_hist"][0] == 1
    assert p("alt_twice_first0")["alt_hist"][1] == 1 and p("alt_twice_first1")["alt_hist"][1] == 1 and p("two_alternatives")["alt_hist"][2] == 1
    assert p("alternatives_64")["alt_hist"][64] == 1 and p("alternatives_64_each_twice")["alt_hist"][64] == 1
    assert p("identity_0")["identity_hist"][0] == 1 and p("identity_100")["identity_hist"][100] == 1 and p("identity_99")["identity_hist"][99] == 1
    assert p("skips_only")["identity_none"] == 1 and p("start_only")["identity_none"] == 1
    assert p("plain")["kind_bases"][0] == 200 and p("plain_with_n")["kind_bases"][1] == 78 and p("plain_empty")["kind_bytes"][0] == 1
    assert p("reversed_main_and_alternative")["main_rev"][1] == 1 and int(p("units_100000")["tuples"][:4].sum()) == 100_000


def test_host_form_equals_the_reference_on_hand_made_streams(hand):
    refs, names, streams, per = hand
    bad = []
    for name, s, want in zip(names, streams, per):
        st, got, _, _ = host_profile([s], refs)
        if st != 0 or E.same(got.as_dict(), want) is not None or E.invariants(got.as_dict()):
            bad.append((name, st, E.same(got.as_dict(), want)))
    assert not bad, bad
    st, got, _, _ = host_profile(streams, refs)
    assert st == 0 and E.same(got.as_dict(), E.profile(streams, refs)) is None


# ---- 3. malformed streams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ES.malformed_host()) + sorted(ES.malformed_device()))
def test_malformed_stream_is_refused_and_nothing_is_added(name, hand):
    refs, _, streams, _ = hand
    bad, why = {**ES.malformed_host(), **ES.malformed_device()}[name]
    with pytest.raises(E.Malformed) as x:
        E.profile_of_read(bad, refs)
    assert x.value.why == why
    good = [streams[3], streams[40], streams[-2]]
    _, acc, _, _ = host_profile(good, refs)
    before = bytes(acc)
    st, acc, read, text = host_profile(good[:2] + [bad] + good[2:], refs, acc)
    assert st == N.CL_E_INVALID and read == 2 and text == why
    assert bytes(acc) == before                                                 # NOTHING of the batch was added, the reads in front of the bad one included


# ---- 4. ABI and the stream --------------------------------------------------------------------------------------------------------------
NAMES = ["cl_edits_clear", "cl_edits_add", "cl_edit_profile", "cl_edit_profile_host", "cl_edit_profile_error", "cl_ctx_set_edit_profile", "cl_ctx_edit_profile",
         "cl_compressor_edit_profile"]


def test_abi_names_and_sizes():
    header = open(os.path.join(ROOT, "include", "colord_hip.h")).read()
    lib = N.load()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in N.exported_names() and hasattr(lib, n)
    from colord_amd import device as D
    for name in ("set_edit_profile", "edit_profile", "edit_profile_of"):
        assert hasattr(D.Context, name)
    assert hasattr(D.Compressor, "edit_profile")
    for n in ("cl_edits_clear", "cl_edits_add", "cl_edit_profile_host", "cl_ctx_set_edit_profile", "cl_ctx_edit_profile", "cl_compressor_edit_profile"):
        assert n in D._OrderedLib._HOST_ONLY
    assert C.sizeof(N.Edits) == 8 * E.WORDS == 8 * 312
    assert [k for k, _ in E.FIELDS] == [k for k, _ in N.Edits._fields_]
    m = re.search(r"typedef struct cl_edits \{(.*?)\} cl_edits;", header, re.S)
    fields = re.findall(r"(\w+)((?:\[\d+\])*)\s*[,;]", m.group(1))
    assert [(n, tuple(int(d) for d in re.findall(r"\d+", dims))) for n, dims in fields] == [(k, (s,) if isinstance(s, int) and s else tuple(s or ())) for k, s in E.FIELDS]
    assert "both carry" in header and "NOT a per-read error rate" in header


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def stamp(path, payload):
    arc = AR.read_archive(os.path.join(ARC, "bovis24_q_4-avg_balanced.colord"))
    AR.write_archive(path, list(arc.values()) + [AR.Stream("hipedits", 0, [(0, payload)])])


def test_hipedits_round_trip_through_info(hand, tmp_path):
    refs, _, streams, _ = hand
    want = E.profile(streams, refs)
    payload = E.pack_hipedits(want)
    assert len(payload) == 8 + 8 * 312 and E.same(E.unpack_hipedits(payload), want) is None
    st, got, _, _ = host_profile(streams, refs)
    assert st == 0 and E.pack_hipedits(got.as_dict()) == payload               # the structure's words in their order ARE the stream's
    arc = str(tmp_path / "s.colord")
    stamp(arc, payload)
    j = run("info", "--edit-profile", "--json", arc)
    assert j.returncode == 0, j.stderr
    o = json.loads(j.stdout)
    back = {k: (np.array(o[k], np.uint64) if s else o[k]) for k, s in E.FIELDS}
    assert E.same(back, want) is None and o["version"] == 1 and "both carry errors" in o["note"]
    d = o["derived"]
    t = [int(x) for x in want["tuples"]]
    aligned = t[E.MATCH] + want["anchor_bases"] + t[E.SUBST] + t[E.INS] + t[E.DEL]
    assert d["aligned_bases"] == aligned and abs(d["sub_rate"] - t[E.SUBST] / aligned) < 1e-8 and abs(d["ins_rate"] - t[E.INS] / aligned) < 1e-8 and abs(d["del_rate"] - t[E.DEL] / aligned) < 1e-8
    ts = int(want["sub"][0, 2] + want["sub"][2, 0] + want["sub"][1, 3] + want["sub"][3, 1])
    assert d["transitions"] == ts and d["transversions"] == t[E.SUBST] - ts
    assert abs(d["ins_run_mean"] - t[E.INS] / int(want["ins_run_hist"].sum())) < 1e-8 and abs(d["ins_in_runs2"] - (t[E.INS] - int(want["ins_run_hist"][1])) / t[E.INS]) < 1e-8
    assert abs(d["anchor_base_share"] - want["anchor_bases"] / int(want["kind_bases"][2])) < 1e-8
    assert abs(d["alts_per_read"] - sum(i * int(c) for i, c in enumerate(want["alt_hist"])) / int(want["kind_reads"][2])) < 1e-8
    cum = np.cumsum(want["identity_hist"].astype(np.int64))
    assert d["identity_median"] == int(np.nonzero(2 * cum >= cum[-1])[0][0])
    t = run("info", "--edit-profile", arc)
    assert t.returncode == 0 and "not a per-read error rate" in t.stdout and "transitions : transversions = %d : %d" % (ts, d["transversions"]) in t.stdout
    i = run("info", arc)
    assert i.returncode == 0 and "edit profile: %d of %d reads coded with an edit script" % (int(want["kind_reads"][2]), want["reads"]) in i.stderr
    plain = run("info", os.path.join(ARC, "bovis24_q_4-avg_balanced.colord"))
    assert plain.returncode == 0 and "edit profile" not in plain.stderr
    none = run("info", "--edit-profile", os.path.join(ARC, "bovis24_q_4-avg_balanced.colord"))
    assert none.returncode == 1 and "no edit profile is stored" in none.stderr


@pytest.mark.parametrize("how", ["version_2", "flags_1", "one_byte_short", "one_byte_more", "header_only"])
def test_a_stream_of_another_shape_is_refused_cleanly(how, tmp_path):
    good = E.pack_hipedits(E.empty())
    payload = {"version_2": struct.pack("<I", 2) + good[4:], "flags_1": good[:4] + struct.pack("<I", 1) + good[8:], "one_byte_short": good[:-1], "one_byte_more": good + b"\0",
               "header_only": good[:8]}[how]
    arc = str(tmp_path / "s.colord")
    stamp(arc, payload)
    r = run("info", "--edit-profile", arc)
    assert r.returncode == 1 and "`hipedits` stream is not one this build reads" in r.stderr
    i = run("info", arc)
    assert i.returncode == 0 and "a `hipedits` stream this build cannot read" in i.stderr


def test_help_names_the_option():
    r = run("compress-ont", "--help")
    assert r.returncode == 0 and "--edit-profile" in r.stderr and "hipedits" in r.stderr and "not a per-read error rate" in r.stderr and "both carry errors" in r.stderr
    assert "info [--report [--json]] [--edit-profile [--json]]" in r.stderr
    r = run("compress-ont", "--edit-profile", "in.fq")
    assert r.returncode == 1 and "expected input and output paths" in r.stderr and "unknown option" not in r.stderr


# ---- the host form under AddressSanitizer and UBSan, as a program of its own ------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    """tests/tools/edits_host_test.cpp: csrc/edits.hpp and csrc/cli/edits_stream.hpp under a host compiler alone (they need no HIP), the sanitizers'
    runtimes linked in; it has its own main and runs as it is, nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("san") / "edits_host_test")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "edits_host_test.cpp"), "-o", exe])
    return exe


def test_host_form_under_sanitizers_equals_the_reference(sanitized_program, hand, tmp_path):
    refs, _, streams, per = hand
    bad = {**ES.malformed_host(), **ES.malformed_device()}
    cases = [[s] for s in streams] + [streams] + [[streams[0], b, streams[1]] for b, _ in bad.values()]
    blob = struct.pack("<I", len(refs)) + np.cumsum([0] + [len(r) for r in refs]).astype("<u8").tobytes() + b"".join(r.tobytes() for r in refs) + struct.pack("<Q", len(cases))
    for c in cases:
        blob += struct.pack("<Q", len(c)) + np.cumsum([0] + [len(s) for s in c]).astype("<u8").tobytes() + b"".join(c)
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    r = subprocess.run([sanitized_program, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"ok: {len(cases)} cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = re.findall(r"^case (.*)$", r.stdout, re.M)
    assert len(lines) == len(cases)
    for want, line in zip(per, lines):
        assert bytes.fromhex(line) == E.pack_hipedits(want)
    assert bytes.fromhex(lines[len(streams)]) == E.pack_hipedits(E.profile(streams, refs))
    for (_, why), line in zip(bad.values(), lines[len(streams) + 1:]):
        assert line == "refused read 1: " + why
