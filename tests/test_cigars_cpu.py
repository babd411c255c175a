"""CPU suite of the CIGARs (cl_cigars_host, `colord_hip compress-* -G genome --mappings --cigars`, `info --mappings --cigar | --sam`).  The
judge is tests/cigars_ref.py (plain Python, written from the definition).  Here: the host twin of the C ABI equals the judge on the hand-made streams of
tests/editstreams.py, tests/overlapstreams.py and tests/cigarstreams.py; the relations between every record of cl_overlaps_host and its operations;
malformed streams are refused as cl_overlaps_host refuses them, with nothing written; the run limit of 2^28 through the shared per-run function; the
`hipcigars` stream through `info` and every refusal of its reader; the host twin under AddressSanitizer and UBSan as a program of its own.  No GPU is
needed."""
import ctypes as C
import os
import re
import struct
import subprocess
import numpy as np
import pytest
from colord_amd import _native as N, archive as AR
import cigars_ref as CR
import cigarstreams as CS
import editstreams as ES
import mappings_ref as MR
import overlaps_ref as OR
import overlapstreams as OS
from test_overlaps_cpu import host_overlaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
GOLDEN_ARC = os.path.join(ROOT, "tests", "golden", "archives", "bovis24_q_4-avg_balanced.colord")
FILL = 0xabababab


def host_cigars(streams, refs, id_limit=0, caps=None):
    """cl_cigars_host -> (status, counts, operations, (n_rec, n_ops), bad read, text of the bad code); caps None: the needs are asked for first"""
    lib = N.load()
    rc = np.ascontiguousarray(np.concatenate(refs) if refs else np.zeros(0, np.uint8), dtype=np.uint8)
    roff = np.cumsum([0] + [len(r) for r in refs]).astype(np.uint64)
    raw = np.frombuffer(b"".join(streams), np.uint8).copy() if streams else np.zeros(0, np.uint8)
    off = np.cumsum([0] + [len(s) for s in streams]).astype(np.uint64)
    bad, code, nr, no = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    args = (rc.ctypes.data, roff.ctypes.data, len(refs), raw.ctypes.data, off.ctypes.data, len(streams), id_limit)
    none = np.zeros(0, np.uint32)
    if caps is None:
        st = lib.cl_cigars_host(*args, None, 0, C.byref(nr), None, 0, C.byref(no), C.byref(bad), C.byref(code))
        if st not in (N.CL_OK, N.CL_E_CAPACITY):
            return st, none, none, (nr.value, no.value), bad.value, lib.cl_cigars_error(code.value).decode()
        caps = (nr.value, no.value)
    rec, ops = np.full(caps[0] + 1, FILL, np.uint32), np.full(caps[1] + 1, FILL, np.uint32)      # one word more than asked for: it must stay as it is
    st = lib.cl_cigars_host(*args, rec.ctypes.data, caps[0], C.byref(nr), ops.ctypes.data, caps[1], C.byref(no), C.byref(bad), C.byref(code))
    assert rec[caps[0]] == FILL and ops[caps[1]] == FILL
    if st != N.CL_OK:
        assert (rec == FILL).all() and (ops == FILL).all(), "something was written although the call failed"
        return st, none, none, (nr.value, no.value), bad.value, lib.cl_cigars_error(code.value).decode()
    return st, rec[:nr.value].copy(), ops[:no.value].copy(), (nr.value, no.value), bad.value, ""


@pytest.fixture(scope="module")
def hand():
    refs = ES.references()
    S = {**ES.hand_made(), **OS.hand_made(), **CS.hand_made()}
    return refs, list(S), list(S.values())


@pytest.fixture(scope="module")
def read_set():
    refs = ES.references()
    streams = CS.read_set()
    return streams, CR.cigars(streams, refs), CR.cigars(streams, refs, CS.ID_LIMIT), OR.records(streams, refs)


# ---- the host twin against the reference -------------------------------------------------------------------------------------------------
def test_host_twin_equals_the_reference_on_hand_made_streams(hand):
    refs, names, streams = hand
    bad = []
    for name, s in zip(names, streams):
        want_rec, want_ops = CR.cigars([s], refs)
        st, rec, ops, _, _, _ = host_cigars([s], refs)
        if st != 0 or not np.array_equal(rec, want_rec) or not np.array_equal(ops, want_ops):
            bad.append((name, st, rec.tolist(), want_rec.tolist()))
    assert not bad, bad[:3]
    want_rec, want_ops = CR.cigars(streams, refs)
    st, rec, ops, _, _, _ = host_cigars(streams, refs)
    assert st == 0 and np.array_equal(rec, want_rec) and np.array_equal(ops, want_ops)


def test_host_twin_equals_the_reference_on_the_read_set(read_set):
    streams, (want_rec, want_ops), (lim_rec, lim_ops), recs = read_set
    refs = ES.references()
    st, rec, ops, _, _, _ = host_cigars(streams, refs)
    assert st == 0 and np.array_equal(rec, want_rec) and np.array_equal(ops, want_ops)
    st, rec, ops, _, _, _ = host_cigars(streams, refs, CS.ID_LIMIT)
    assert st == 0 and np.array_equal(rec, lim_rec) and np.array_equal(ops, lim_ops)
    assert np.array_equal(lim_rec == 0, recs[:, 1] >= CS.ID_LIMIT)                         # the zeros are exactly the records at or past the limit
    assert CR.invariants(recs, rec, ops, zero_ok=True) == []
    cut = len(streams) // 3                                                              # two calls give the same as one
    _, ra, oa, _, _, _ = host_cigars(streams[:cut], refs)
    _, rb, ob, _, _, _ = host_cigars(streams[cut:], refs)
    assert np.array_equal(np.concatenate([ra, rb]), want_rec) and np.array_equal(np.concatenate([oa, ob]), want_ops)


def test_relations_hold_against_the_overlap_records(hand, read_set):
    """cl_overlaps_host's records, cl_cigars_host's operations: two walks of the library, held against each other by the judge's relations"""
    refs, _, streams = hand
    for sset in (streams, read_set[0]):
        st, recs, _, _, _ = host_overlaps(sset, refs)
        st2, rec, ops, _, _, _ = host_cigars(sset, refs)
        assert st == 0 and st2 == 0 and len(recs) == len(rec) > 100
        assert CR.invariants(recs, rec, ops) == []
    broken = ops.copy(); broken[5] += 1 << 4                                               # (the judge's relations do see a base too many)
    assert CR.invariants(recs, rec, broken) != []


def test_hand_made_streams_cover_the_operations(hand):
    refs, _, streams = hand
    rec, ops = CR.cigars(streams, refs)
    cgs = CR.split(rec, ops)
    assert {op for cg in cgs for op, _ in cg} == {CR.OP_I, CR.OP_D, CR.OP_EQ, CR.OP_X}
    assert max(n for cg in cgs for op, n in cg if op == CR.OP_I) >= 70 and max(n for cg in cgs for op, n in cg if op == CR.OP_D) >= 70
    assert min(len(cg) for cg in cgs) == 1 and max(len(cg) for cg in cgs) >= 301


def test_capacity_protocol(read_set):
    streams, (want_rec, want_ops), _, _ = read_set
    refs = ES.references()
    for caps in ((len(want_rec) - 1, len(want_ops)), (len(want_rec), len(want_ops) - 1), (0, 0)):
        st, _, _, need, _, _ = host_cigars(streams, refs, caps=caps)
        assert st == N.CL_E_CAPACITY and need == (len(want_rec), len(want_ops))


# ---- malformed streams -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ES.malformed_host()) + sorted(ES.malformed_device()))
def test_malformed_stream_is_refused_as_the_overlaps_refuse_it(name, hand):
    refs, _, streams = hand
    bad, why = {**ES.malformed_host(), **ES.malformed_device()}[name]
    with pytest.raises(OR.Malformed) as x:
        CR.cigars_of_read(bad, refs)
    assert x.value.why == why
    good = [streams[3], streams[40], streams[-2]]
    sset = good[:2] + [bad] + good[2:]
    for caps in (None, (1000, 100000)):                                                  # with room for everything: still nothing written
        st, _, _, need, read, text = host_cigars(sset, refs, caps=caps)
        assert st == N.CL_E_INVALID and need == (0, 0) and read == 2 and text == why
    st, _, n, read, text = host_overlaps(sset, refs)
    assert (st, read, text) == (N.CL_E_INVALID, 2, why)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
NAMES = ["cl_cigars_of", "cl_cigars_host", "cl_cigars_error", "cl_ctx_set_cigars", "cl_ctx_cigars", "cl_compressor_cigars"]


def test_abi_names():
    header = open(os.path.join(ROOT, "include", "colord_hip.h")).read()
    lib = N.load()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in N.exported_names() and hasattr(lib, n)
    from colord_amd import device as D
    for name in ("set_cigars", "cigars", "cigars_of"):
        assert hasattr(D.Context, name)
    assert hasattr(D.Compressor, "cigars")
    for n in NAMES[1:]:
        assert n in D._OrderedLib._HOST_ONLY
    assert lib.cl_cigars_error(256).decode() == CR.RUN_TEXT and lib.cl_cigars_error(3).decode() == "tuple type not allowed inside an edit script"
    assert "REVERSED BY WHOEVER PRINTS" in header


# ---- the stream through `info` -----------------------------------------------------------------------------------------------------------
SEQ_LEN, SEQ_NAMES = [5000, 0, 3000], ["chrA", "empty", ""]


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def stamp(path, mappings, cigars):
    arc = AR.read_archive(GOLDEN_ARC)
    extra = [AR.Stream("hipmappings", 0, [(0, mappings)])] + ([AR.Stream("hipcigars", 0, [(0, cigars)])] if cigars is not None else [])
    AR.write_archive(path, list(arc.values()) + extra)


def made_up(seed=7, n=40):
    """lifted mapping records over the 24 reads of a golden archive with CIGARs that fit them: (records, counts, operations)"""
    rng = np.random.default_rng(seed)
    recs, cgs = [], []
    for q in np.sort(rng.integers(0, 24, n)):
        ops = [int(rng.choice([CR.OP_EQ, CR.OP_X]))]
        for _ in range(int(rng.integers(0, 9))):
            ops.append(int(rng.choice([o for o in (CR.OP_I, CR.OP_D, CR.OP_EQ, CR.OP_X) if o != ops[-1]])))
        if ops[-1] in (CR.OP_I, CR.OP_D):
            ops.append(CR.OP_EQ)
        cg = [(op, int(rng.integers(1, 40))) for op in ops]
        tot = lambda which: sum(k for op, k in cg if op in which)
        t = int(rng.choice([0, 2]))
        qs, ts, m = int(rng.integers(0, 50)), int(rng.integers(0, 500)), tot((CR.OP_EQ,))
        qe, te = qs + tot((CR.OP_EQ, CR.OP_X, CR.OP_I)), ts + tot((CR.OP_EQ, CR.OP_X, CR.OP_D))
        recs.append((int(q), t, qe + int(rng.integers(0, 3)), SEQ_LEN[t], qs, qe, ts, te, m, tot((CR.OP_X,)), int(rng.integers(0, m + 1)), MR.GENOME | int(rng.integers(0, 4))))
        cgs.append(cg)
    return np.array(recs, np.uint32), np.array([len(cg) for cg in cgs], np.uint32), np.array([w for cg in cgs for w in CR.words(cg)], np.uint32)


def test_hipcigars_round_trip_through_info(tmp_path):
    recs, rec_ops, ops = made_up()
    assert CR.invariants(recs, rec_ops, ops) == [] and set((recs[:, 11] & 1).tolist()) == {0, 1} and (recs[:, 4] > 0).any() and (recs[:, 5] < recs[:, 2]).any()
    payload = CR.pack_hipcigars(rec_ops, ops)
    assert len(payload) == CR.HEAD + 4 * (len(rec_ops) + len(ops))
    arc = str(tmp_path / "c.colord")
    stamp(arc, MR.pack(recs, SEQ_LEN, SEQ_NAMES, 100, 30), payload)
    r = run("info", "--mappings", "--cigar", arc)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == CR.paf_lines(recs, rec_ops, ops, SEQ_LEN, SEQ_NAMES)
    plain = run("info", "--mappings", arc)                                               # the PAF of today, and the same lines with one column more
    assert plain.returncode == 0 and plain.stdout.splitlines() == MR.paf_lines(recs, SEQ_LEN, SEQ_NAMES)
    assert [line.rsplit("\t", 1)[0] for line in r.stdout.splitlines()] == plain.stdout.splitlines()
    for line, rec, cg in zip(r.stdout.splitlines(), recs, CR.split(rec_ops, ops)):        # reversed for `-`, as it is for `+`
        tag = line.split("\t")[15]
        assert tag == "cg:Z:" + CR.text(cg[::-1] if line.split("\t")[4] == "-" else cg)
    blocks = sorted(OR.block(x) for x in recs)
    mid = blocks[len(blocks) // 2]
    r = run("info", "--mappings", "--cigar", "--min-block", str(mid), arc)               # a hidden record takes its CIGAR with it
    assert r.returncode == 0 and r.stdout.splitlines() == CR.paf_lines(recs, rec_ops, ops, SEQ_LEN, SEQ_NAMES, min_block=mid) and 0 < len(r.stdout.splitlines()) < len(recs)
    r = run("info", "--mappings", "--sam", arc)
    assert r.returncode == 0 and r.stdout.splitlines() == CR.sam_lines(recs, rec_ops, ops, SEQ_LEN, SEQ_NAMES)
    body = [line.split("\t") for line in r.stdout.splitlines() if not line.startswith("@")]
    assert r.stdout.splitlines()[:4] == ["@HD\tVN:1.6\tSO:unknown", "@SQ\tSN:chrA\tLN:5000", "@SQ\tSN:empty\tLN:0", "@SQ\tSN:2\tLN:3000"] and len(body) == len(recs)
    for row, rec in zip(body, recs):
        assert len(row) == 12 and int(row[3]) == rec[6] + 1 and row[4] == "255" and row[6:11] == ["*", "0", "0", "*", "*"]
        assert sum(n for c, n in CR.parse_text(row[5]) if c in "=XIH") == rec[2]          # the query length with its hard clips is qlen
    assert {int(row[1]) for row in body} == {0, 16, 2048, 2064}
    dec = str(tmp_path / "d.fastq")
    assert run("decompress", arc, dec).returncode == 0 and run("check", arc).returncode == 0      # `decompress` and `check` ignore the stream
    ids = [line[1:].split()[0] for line in open(dec).read().splitlines()[0::4]]
    r = run("info", "--mappings", "--sam", "--names", arc)
    assert r.returncode == 0 and r.stdout.splitlines() == CR.sam_lines(recs, rec_ops, ops, SEQ_LEN, SEQ_NAMES, read_names=ids)
    r = run("info", "--mappings", "--cigar", "--names", arc)
    assert r.returncode == 0 and r.stdout.splitlines() == CR.paf_lines(recs, rec_ops, ops, SEQ_LEN, SEQ_NAMES, read_names=ids)
    i = run("info", arc)
    assert i.returncode == 0 and "cigars: %d operations of %d mapping records" % (len(ops), len(recs)) in i.stderr
    none = str(tmp_path / "n.colord")
    stamp(none, MR.pack(recs, SEQ_LEN, SEQ_NAMES, 100, 30), None)
    for form in ("--cigar", "--sam"):
        r = run("info", "--mappings", form, none)
        assert r.returncode == 1 and "no CIGARs are stored" in r.stderr and r.stdout == ""
    assert "cigars" not in run("info", none).stderr
    stamp(none, MR.pack(recs[:0], SEQ_LEN, SEQ_NAMES, 100, 30), CR.pack_hipcigars([], []))
    r = run("info", "--mappings", "--cigar", none)
    assert r.returncode == 0 and r.stdout == ""


def bad_payloads():
    recs, rec_ops, ops = made_up()
    good = CR.pack_hipcigars(rec_ops, ops)
    first = CR.split(rec_ops, ops)[0]

    def with_ops(i, new):
        o = ops.copy(); o[i] = new
        return CR.pack_hipcigars(rec_ops, o)
    shifted = rec_ops.copy(); shifted[0] += 1; shifted[1] -= 1
    gap = next(i for i, w in enumerate(ops.tolist()) if w & 0xf in (CR.OP_I, CR.OP_D))
    P = {"version_2": CR.pack_hipcigars(rec_ops, ops, version=2), "operation_size_8": CR.pack_hipcigars(rec_ops, ops, op_bytes=8), "one_byte_short": good[:-1], "one_operation_short": good[:-4],
         "head_cut": good[:20], "records_without_bytes": CR.pack_hipcigars(rec_ops, ops, records=1 << 40), "operations_one_more": CR.pack_hipcigars(rec_ops, ops, operations=len(ops) + 1),
         "one_record_more": CR.pack_hipcigars(np.append(rec_ops, 0), ops), "one_record_fewer": CR.pack_hipcigars(rec_ops[:-1], ops[:len(ops) - int(rec_ops[-1])]),
         "counts_do_not_add_up": CR.pack_hipcigars(np.append(rec_ops[:-1], rec_ops[-1] + 1), ops), "counts_shifted": CR.pack_hipcigars(shifted, ops),
         "query_length": with_ops(0, ops[0] + (1 << 4)), "first_is_an_insertion": with_ops(0, (int(ops[0]) & ~0xf) | CR.OP_I),
         "matches_as_subst": with_ops(0, (int(ops[0]) & ~0xf) | (CR.OP_X if first[0][0] == CR.OP_EQ else CR.OP_EQ)), "unknown_code": with_ops(gap, (int(ops[gap]) & ~0xf) | 3),
         "length_0": with_ops(gap, int(ops[gap]) & 0xf)}
    if len(first) > 1:
        P["neighbours_equal"] = with_ops(1, (int(ops[1]) & ~0xf) | first[0][0])
    return recs, P


@pytest.mark.parametrize("how", sorted(bad_payloads()[1]))
def test_a_stream_the_reader_must_refuse_gives_exit_1(how, tmp_path):
    recs, P = bad_payloads()
    arc = str(tmp_path / "s.colord")
    stamp(arc, MR.pack(recs, SEQ_LEN, SEQ_NAMES, 100, 30), P[how])
    for form in ("--cigar", "--sam"):
        r = run("info", "--mappings", form, arc)
        assert r.returncode == 1 and "`hipcigars` stream is not one this build reads" in r.stderr and r.stdout == "", how
    assert run("info", "--mappings", arc).returncode == 0                                # the mappings themselves are printed as before
    i = run("info", arc)
    assert i.returncode == 0 and ("a `hipcigars` stream this build cannot read" in i.stderr) == (how in ("version_2", "operation_size_8", "head_cut"))


def test_help_and_refused_combinations(tmp_path):
    r = run("compress-ont", "--help")
    assert r.returncode == 0 and "--cigars" in r.stderr and "hipcigars" in r.stderr and "THE STREAM IS LARGER THAN THE `dna` STREAM" in r.stderr
    assert "info --mappings --cigar | --mappings --sam [--min-block N] [--names] archive.colord" in r.stderr
    out = str(tmp_path / "out.colord")
    for extra in ([], ["-G", "genome.fa"], ["-G", "genome.fa", "--pileup"]):
        r = run("compress-ont", "--cigars", *extra, "in.fq", out)
        assert r.returncode == 1 and "--cigars needs --mappings" in r.stderr and not os.path.exists(out), r.stderr
    for extra, text in ((["--gpus", "2"], "--mappings is not available with --gpus > 1"), (["--domains", "2"], "--mappings is not available with --domains > 1")):
        r = run("compress-ont", "-G", "genome.fa", "--mappings", "--cigars", *extra, "in.fq", out)
        assert r.returncode == 1 and text in r.stderr and not os.path.exists(out), r.stderr
    for args in (["--cigar"], ["--sam"], ["--mappings", "--cigar", "--sam"], ["--mappings", "--cigar", "--summary"], ["--mappings", "--sam", "--coverage", "10"], ["--overlaps", "--cigar"],
                 ["--mappings", "--sam", "--json"]):
        r = run("info", *args, GOLDEN_ARC)
        assert r.returncode == 1 and "usage" in r.stderr, args


# ---- the host twin under AddressSanitizer and UBSan, as a program of its own ------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    """tests/tools/cigars_host_test.cpp: csrc/cigars.hpp and csrc/cli/cigars_stream.hpp under a host compiler alone (they need no HIP), the
    sanitizers' runtimes linked in; it has its own main and runs as it is, nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("san") / "cigars_host_test")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "cigars_host_test.cpp"), "-o", exe])
    return exe


def test_host_twin_under_sanitizers_equals_the_reference(sanitized_program, hand, read_set, tmp_path):
    refs, _, streams = hand
    bad = {**ES.malformed_host(), **ES.malformed_device()}
    sets = [streams, read_set[0]]
    cases = [[s] for s in streams] + sets + [[streams[0], b, streams[1]] for b, _ in bad.values()]
    blob = struct.pack("<I", len(refs)) + np.cumsum([0] + [len(r) for r in refs]).astype("<u8").tobytes() + b"".join(r.tobytes() for r in refs) + struct.pack("<Q", len(cases))
    for c in cases:
        blob += struct.pack("<Q", len(c)) + np.cumsum([0] + [len(s) for s in c]).astype("<u8").tobytes() + b"".join(c)
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    r = subprocess.run([sanitized_program, str(path), str(CS.ID_LIMIT)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"ok: {len(cases)} cases" in r.stdout and "run limit ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = re.findall(r"^case (.*)$", r.stdout, re.M)
    assert len(lines) == len(cases)
    for c, line in zip(cases[:len(streams) + len(sets)], lines):
        assert bytes.fromhex(line) == CR.pack_hipcigars(*CR.cigars(c, refs))
    for (_, why), line in zip(bad.values(), lines[len(streams) + len(sets):]):
        assert line == "refused read 1: " + why
