"""CPU suite of the coded CIGARs (cl_cigars_pack_host, cl_cigars_unpack_host, `hipcigars` version 2).  The judge is
tests/cigarcoder_ref.py (plain Python, written from the definition).  Here: the host twin's bytes equal the judge's on the constructed words of
tests/cigarcodercases.py; the decoder gives the words back; every refusal of the decoder, by corrupting one field of a segment at a time; version 1
of the stream still reads and version 2 round-trips through `info`; the host twin, the decoder and the reader under AddressSanitizer and UBSan as a
program of its own.  No GPU is needed."""
import ctypes as C
import os
import re
import struct
import subprocess
import numpy as np
import pytest
from colord_amd import _native as N, device as D
import cigarcoder_ref as CC
import cigarcodercases as K
import cigars_ref as CR
import mappings_ref as MR
from test_cigars_cpu import made_up, stamp, run, SEQ_LEN, SEQ_NAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_SIZES, R_HEADER, R_TABLE, R_TABLE_SUM, R_TOT0, R_SYMBOL, R_ESCAPES, R_ESC_VALUE, R_PART_END = range(1, 10)


@pytest.fixture(scope="module")
def judged():
    return {name: (w, p, s, CC.pack(list(w), p, s)) for name, (w, p, s) in K.cases().items()}


def check(data):
    """(cl_cigars_check_host's code, cl_cigars_unpack_host's status) of the bytes, with a guard byte on either side of them"""
    lib = N.load()
    raw = np.frombuffer(b"\xee" + data + b"\xee", np.uint8).copy()
    no = C.c_uint64(5)
    st = lib.cl_cigars_unpack_host(raw.ctypes.data + 1, len(data), None, 0, C.byref(no))
    return lib.cl_cigars_check_host(raw.ctypes.data + 1, len(data)), st


def test_host_twin_equals_the_judge_on_every_case(judged):
    bad = [name for name, (w, p, s, want) in judged.items() if D.cigars_pack_host(w, p, s) != want]
    assert not bad, bad
    w = K.ont_like(5000)
    assert D.cigars_pack_host(w) == CC.pack(list(w))                                      # the default knobs
    assert judged["n0"][3] == b"" and len(judged) >= 20


def test_the_decoder_gives_the_words_back(judged):
    for name, (w, p, s, want) in judged.items():
        assert np.array_equal(D.cigars_unpack_host(want), w), name
        assert np.array_equal(CC.unpack(want), w), name
        assert check(want)[0] == 0
    n_ops, part_ops, n_esc, _ = struct.unpack_from("<4I", judged["escape_boundary"][3])
    assert (n_ops, part_ops, n_esc) == (5, K.PART, 3)                                    # 255 is a symbol; 256, 257 and 2^28 - 1 escape


def test_words_that_are_no_operations_are_refused_with_the_first_index():
    for name, (w, at) in K.bad_cases().items():
        with pytest.raises(CC.Invalid) as j:
            CC.pack(list(w), K.PART, K.SEG)
        with pytest.raises(ValueError) as h:
            D.cigars_pack_host(w, K.PART, K.SEG)
        assert j.value.index == at and "word %d is" % at in str(h.value), name


def corrupted():
    """name -> (bytes, the refusal's code or None where only a refusal is known): one field of one segment changed at a time"""
    w = (K.mixed(40, 21) & 0xf) | (np.arange(40, dtype=np.uint32) % 3 + 1) << 4
    w[7] = 1000 << 4 | K.EQ; w[30] = 300 << 4 | K.D
    counts, escapes, parts = CC.segment_pieces(list(w), K.PART)
    seg = lambda **kw: CC.segment_bytes(len(w), K.PART, kw.pop("counts", counts), kw.pop("escapes", escapes), kw.pop("parts", parts), **kw)
    good = seg()
    assert good == CC.pack(list(w), K.PART, K.SEG) and escapes == [1000, 300]
    sizes = [len(p) for p in parts]
    P = {"one_byte_short": (good[:-1], R_SIZES), "head_cut": (good[:12], R_SIZES), "a_part_size_past_the_bytes": (seg(sizes=sizes[:-1] + [sizes[-1] + 1]), R_SIZES),
         "sizes_without_bytes": (struct.pack("<4I", 1 << 20, 1, 0, 0), R_SIZES), "table_bytes_past_the_bytes": (good[:12] + struct.pack("<I", 1 << 30) + good[16:], R_SIZES),
         "no_operations": (struct.pack("<4I", 0, 16, 0, 0), R_HEADER), "too_many_operations": (struct.pack("<I", (1 << 20) + 1) + good[4:], R_HEADER), "part_ops_0": (good[:4] + struct.pack("<I", 0) + good[8:], R_HEADER)}
    c = list(counts); c[CC.op_bin(4, 0)] += 1
    P["table_one_more"] = (seg(counts=c), R_TABLE_SUM)
    P["table_cut"] = (seg(table=b"".join(CC.leb128(x) for x in counts)[:-1]), R_TABLE)
    P["table_value_never_ends"] = (seg(table=b"\x80" * 1044), R_TABLE)
    P["table_one_value_more"] = (seg(table=b"".join(CC.leb128(x) for x in counts) + b"\x00"), R_TABLE)
    P["escape_below_256"] = (seg(escapes=[255, 300]), R_ESC_VALUE)
    P["escape_past_the_longest_run"] = (seg(escapes=[1000, 1 << 28]), R_ESC_VALUE)
    P["an_escape_left_over"] = (seg(escapes=escapes + [400]), R_ESCAPES)
    P["escapes_run_out"] = (seg(escapes=escapes[:1]), R_ESCAPES)
    P["a_part_longer_than_it_is"] = (seg(parts=[parts[0] + b"\x00"] + parts[1:]), R_PART_END)
    P["a_part_shorter_than_it_is"] = (seg(parts=[parts[0][:-1]] + parts[1:]), None)
    P["a_part_below_its_8_end_bytes"] = (seg(parts=[parts[0][:7]] + parts[1:]), R_PART_END)
    P["a_part_of_ff"] = (seg(parts=[b"\xff" * len(parts[0])] + parts[1:]), R_SYMBOL)
    P["two_segments_second_cut"] = (good + good[:-3], R_SIZES)
    # a context in use with the total 0: = and X alternate in one part; the row `after X` moved to the row `after I` keeps every sum
    alt = K.words_of([K.EQ, K.X] * 5, [1] * 10)
    ac, ae, ap = CC.segment_pieces(list(alt), K.PART)
    moved = list(ac)
    for o in range(4):
        moved[CC.op_bin(0, o)] += moved[CC.op_bin(3, o)]; moved[CC.op_bin(3, o)] = 0
    assert CC.segment_bytes(10, K.PART, ac, ae, ap) == CC.pack(list(alt), K.PART, K.SEG)
    P["a_context_in_use_with_total_0"] = (CC.segment_bytes(10, K.PART, moved, ae, ap), R_TOT0)
    return good, P


def test_the_corrupted_segments_are_made_of_a_good_one():
    good, P = corrupted()
    assert check(good) == (0, N.CL_E_CAPACITY) and len(P) >= 20                             # (the good one decodes: 40 words, no room given)
    assert check(good + good) == (0, N.CL_E_CAPACITY)


@pytest.mark.parametrize("how", sorted(corrupted()[1]))
def test_every_refusal_stays_a_refusal(how):
    data, code = corrupted()[1][how]
    got, st = check(data)
    assert st == N.CL_E_INVALID and got != 0 and (code is None or got == code), (how, got, N.load().cl_cigars_refusal(got))
    with pytest.raises(CC.Refused):
        CC.unpack(data)
    with pytest.raises(ValueError):
        D.cigars_unpack_host(data)


# ---- the stream through `info` -----------------------------------------------------------------------------------------------------------
def test_version_1_still_reads_and_version_2_round_trips(tmp_path):
    recs, rec_ops, ops = made_up()
    maps = MR.pack(recs, SEQ_LEN, SEQ_NAMES, 100, 30)
    v1, v2 = str(tmp_path / "v1.colord"), str(tmp_path / "v2.colord")
    stamp(v1, maps, CR.pack_hipcigars(rec_ops, ops))
    seg = D.cigars_pack_host(ops, 16, 64)
    n_seg = -(-len(ops) // 64)
    assert seg == CC.pack(list(ops), 16, 64) and n_seg > 1
    payload = CC.pack_hipcigars2(rec_ops, seg, len(ops), n_seg)
    stamp(v2, maps, payload)
    for form in ("--cigar", "--sam"):
        a, b = run("info", "--mappings", form, v1), run("info", "--mappings", form, v2)
        assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and len(a.stdout.splitlines()) >= len(recs), b.stderr
    assert run("info", "--mappings", "--cigar", v2).stdout.splitlines() == CR.paf_lines(recs, rec_ops, ops, SEQ_LEN, SEQ_NAMES)
    i1, i2 = run("info", v1).stderr, run("info", v2).stderr
    line = "cigars: %d operations of %d mapping records" % (len(ops), len(recs))
    assert line in i1 and "coded" not in i1
    assert line + ", coded: %d bytes in %d segments, %.3f bytes per operation, %d escapes" % (len(seg), n_seg, len(seg) / len(ops), 0) in i2
    counts, escapes, parts = CC.segment_pieces(list(ops[:64]), 16)
    at = CC.HEAD2 + 4 * len(rec_ops) + 16 + 4 * len(parts) + sum(len(CC.leb128(c)) for c in counts)      # the first byte of the first part (of a part's last 8 bytes some decide nothing)
    assert payload[at:at + len(parts[0])] == parts[0]
    bad = {"a_part_byte": payload[:at] + bytes([payload[at] ^ 0xff]) + payload[at + 1:], "one_byte_short": payload[:-1], "segments_one_more": payload[:24] + struct.pack("<Q", n_seg + 1) + payload[32:],
           "operations_one_more": payload[:16] + struct.pack("<Q", len(ops) + 1) + payload[24:], "segment_bytes_one_more": payload[:32] + struct.pack("<Q", len(seg) + 1) + payload[40:],
           "a_count_moved": CC.pack_hipcigars2(np.concatenate([[rec_ops[0] + 1, rec_ops[1] - 1], rec_ops[2:]]), seg, len(ops), n_seg),
           "other_operations": CC.pack_hipcigars2(rec_ops, D.cigars_pack_host(ops[::-1].copy(), 16, 64), len(ops), n_seg), "version_3": struct.pack("<I", 3) + payload[4:], "head_cut": payload[:30]}
    for how, p in bad.items():
        arc = str(tmp_path / "bad.colord")
        stamp(arc, maps, p)
        r = run("info", "--mappings", "--cigar", arc)
        assert r.returncode == 1 and "`hipcigars` stream is not one this build reads" in r.stderr and r.stdout == "", how
        assert run("info", "--mappings", arc).returncode == 0


def test_help_names_and_refused_combinations(tmp_path):
    r = run("compress-ont", "--help")
    assert r.returncode == 0 and "--cigars-coded" in r.stderr and "version 2" in r.stderr and "THE STREAM IS LARGER THAN THE `dna` STREAM" in r.stderr
    out = str(tmp_path / "o.colord")
    for extra in ([], ["-G", "genome.fa"], ["-G", "genome.fa", "--mappings"]):
        r = run("compress-ont", "--cigars-coded", *extra, "in.fq", out)
        assert r.returncode == 1 and ("--cigars-coded needs --cigars" in r.stderr) and not os.path.exists(out), r.stderr
    for extra, text in ((["--gpus", "2"], "--mappings is not available with --gpus > 1"), (["--domains", "2"], "--mappings is not available with --domains > 1")):
        r = run("compress-ont", "-G", "genome.fa", "--mappings", "--cigars", "--cigars-coded", *extra, "in.fq", out)
        assert r.returncode == 1 and text in r.stderr and not os.path.exists(out), r.stderr
    header = open(os.path.join(ROOT, "include", "colord_hip.h")).read()
    lib = N.load()
    for n in ("cl_cigars_pack", "cl_cigars_pack_host", "cl_cigars_unpack_host", "cl_cigars_check_host", "cl_cigars_refusal", "cl_ctx_set_cigars_coded", "cl_ctx_cigars_coded", "cl_compressor_cigars_coded"):
        assert re.search(r"\b%s\(" % n, header) and n in N.exported_names() and hasattr(lib, n), n
    for name in ("cigars_pack", "set_cigars_coded", "cigars_coded"):
        assert hasattr(D.Context, name)
    assert hasattr(D.Compressor, "cigars_coded") and lib.cl_cigars_refusal(R_PART_END).decode() == "a part does not end at its size"


# ---- the host twin, the decoder and the reader under AddressSanitizer and UBSan, as a program of its own ----------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    """tests/tools/cigarcoder_host_test.cpp: csrc/cigar_coder.hpp, csrc/host_coder.hpp and csrc/cli/cigars_stream.hpp under a host compiler alone
    (they need no HIP), the sanitizers' runtimes linked in; it has its own main and runs as it is, nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("san") / "cigarcoder_host_test")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "cigarcoder_host_test.cpp"), "-o", exe])
    return exe


def test_host_twin_and_decoder_under_sanitizers(sanitized_program, judged, tmp_path):
    cases = [(w, p, s) for w, p, s, _ in judged.values()] + [(w, K.PART, K.SEG) for w, _ in K.bad_cases().values()]
    _, P = corrupted()
    blob = struct.pack("<Q", len(cases))
    for w, p, s in cases:
        blob += struct.pack("<2IQ", p, s, len(w)) + np.ascontiguousarray(w, "<u4").tobytes()
    blob += struct.pack("<Q", len(P))
    for how in sorted(P):
        blob += struct.pack("<Q", len(P[how][0])) + P[how][0]
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    r = subprocess.run([sanitized_program, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "stream ok" in r.stdout and "ok: %d cases, %d corrupted segments" % (len(cases), len(P)) in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    lines = re.findall(r"^case (.*)$", r.stdout, re.M)
    assert len(lines) == len(cases)
    for (_, _, _, want), line in zip(judged.values(), lines):
        assert bytes.fromhex(line) == want
    for (_, at), line in zip(K.bad_cases().values(), lines[len(judged):]):
        assert line == "refused word %d" % at
    codes = [int(x) for x in re.findall(r"^bad (\d+) ", r.stdout, re.M)]
    assert len(codes) == len(P) and all(c != 0 and (P[how][1] is None or c == P[how][1]) for how, c in zip(sorted(P), codes))
