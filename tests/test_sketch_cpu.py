"""CPU suite of the k-mer MinHash sketch: the judge (tests/sketch_ref.py) against the goldens of the unmodified reference and the
judge of the count spectrum, the ABI and the host-side accumulator, the `hipsketch` stream through `colord_hip info --sketch`, and `colord_hip dist`
on stamped archives."""
import ctypes as C
import json
import os
import re
import subprocess
import numpy as np
import pytest
from colord_amd import _native as N, archive as AR
from util import PLAIN_CONFIGS, golden
import kspec_ref as K
import sketch_ref as S
from test_kspec_cpu import golden_kmers, judged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
ARC = os.path.join(ROOT, "tests", "golden", "archives")


# ---- 1. the judge ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", PLAIN_CONFIGS)
def test_judge_on_the_goldens(cfg):
    h = K.hist(judged(cfg))
    assert not judged(cfg)["big"].any()
    for m in (1, 2, 3):
        s = S.from_kmers(golden_kmers(cfg), 500, m)
        assert s["qualifying"] == sum(h[m:])
        assert len(s["hash"]) == len(s["count"]) == min(500, s["qualifying"])
        assert np.all(s["hash"][1:] > s["hash"][:-1]) and np.all(s["count"] >= m)
        # every entry is a k-mer of the input with that count
        keys, counts = np.unique(golden_kmers(cfg), return_counts=True)
        at = np.searchsorted(keys, S.unhash(s["hash"]))
        assert np.array_equal(keys[at], S.unhash(s["hash"])) and np.array_equal(counts[at].astype(np.uint64), s["count"])


def test_numbers_of_c1_ont_default():
    km = golden_kmers("c1_ont_default")
    assert [S.from_kmers(km, 500, m)["qualifying"] for m in (1, 2, 3)] == [34041, 2522, 454]
    whole = S.from_kmers(km, 10000, 2)
    assert len(whole["hash"]) == 2522                                           # complete at the default size
    assert np.bincount((whole["hash"] >> np.uint64(S.BIN_SHIFT)).astype(np.int64), minlength=4096).max() <= 5


def test_unhash_inverts_hash():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.integers(0, 2 ** 63, 5000).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, 5000).astype(np.uint64),
                        np.array([0, 1, S.SALT, S.M64, 2 ** 63, 2 ** 56 - 1], np.uint64)])
    assert np.array_equal(S.unhash(S.hash(x)), x) and np.array_equal(S.hash(S.unhash(x)), x)
    assert S.unhash(S.hash(12345)) == 12345 and S.hash(S.unhash(0)) == 0 and S.hash(S.unhash(S.M64)) == S.M64
    assert S.hash(S.SALT) == 0                                                  # (fmix64 maps 0 to 0)
    assert len(np.unique(S.hash(x))) == len(np.unique(x))


def test_merge_rule():
    km = golden_kmers("c1_ont_default")
    keys, counts = np.unique(km, return_counts=True)
    for size, m in ((500, 2), (10000, 2), (300, 1)):
        whole = S.from_runs(keys, counts, size, m)
        half = len(keys) // 2                                                   # disjoint key ranges, as the counter's and the ranks'
        both = S.merge(S.from_runs(keys[:half], counts[:half], size, m), S.from_runs(keys[half:], counts[half:], size, m))
        assert S.same(both, whole) is None, S.same(both, whole)
    # equal hashes add their counts (independent k-mer sets)
    a = S.from_runs([5, 6, 7], [2, 3, 4], 10, 2)
    b = S.from_runs([6, 7, 8], [10, 20, 30], 10, 2)
    ab = S.merge(a, b)
    assert ab["qualifying"] == 6 and S.same(ab, dict(S.from_runs([5, 6, 7, 8], [2, 13, 24, 30], 10, 2), qualifying=6)) is None
    two = S.merge(S.from_runs([5, 6, 7], [2, 3, 4], 2, 2), S.from_runs([6, 7, 8], [10, 20, 30], 2, 2))
    assert S.same(two, dict(S.from_runs([5, 6, 7, 8], [2, 13, 24, 30], 2, 2), qualifying=6)) is None


def test_pack_round_trip():
    s = S.from_kmers(golden_kmers("c1_ont_default"), 500, 2)
    h, t = S.unpack(S.pack(s, 20, 12, sets=3, flags=1))
    assert [h[x] for x in S.HEADER] == [1, 1, 20, 12, 2, 500, 3, 0] and S.same(s, t) is None and len(S.pack(s, 20, 12)) == 48 + 16 * 500


# ---- 2. the ABI and the accumulator on the host ------------------------------------------------------------------------------------------
NAMES = ["cl_sketch_hash", "cl_sketch_create", "cl_sketch_free", "cl_sketch_info", "cl_sketch_entries", "cl_sketch_merge", "cl_kmer_sketch_runs",
         "cl_ctx_set_kmer_sketch", "cl_ctx_kmer_sketch", "cl_compressor_kmer_sketch"]


def test_abi_names_sizes_and_the_hash():
    header = open(os.path.join(ROOT, "include", "colord_hip.h")).read()
    lib = N.load()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in N.exported_names() and hasattr(lib, n)
    from colord_amd import device as D
    for name in ("set_kmer_sketch", "kmer_sketch", "kmer_sketch_runs"):
        assert hasattr(D.Context, name)
    assert C.sizeof(N.SketchEntry) == 16 and re.search(r"typedef struct cl_sketch_entry \{ uint64_t hash, count; \} cl_sketch_entry;", header)
    assert "0x9E3779B97F4A7C15" in header and "no counterpart in the reference" in header
    rng = np.random.default_rng(2)
    xs = [0, 1, S.SALT, S.M64, 2 ** 40 - 1] + [int(v) for v in rng.integers(0, 2 ** 63, 200)]
    assert [lib.cl_sketch_hash(x) for x in xs] == [S.hash(x) for x in xs]


def test_the_accumulator_merges_as_the_judge():
    a, b = S.from_runs([5, 6, 7], [2, 3, 4], 3, 2), S.from_runs([6, 7, 8, 9], [10, 20, 30, 40], 3, 2)
    acc = N.Sketch(3, 2)
    assert S.same(acc.as_dict(), S.empty(3, 2)) is None
    acc.merge(a["hash"], a["count"], a["qualifying"])
    assert S.same(acc.as_dict(), a) is None
    acc.merge(b["hash"], b["count"], b["qualifying"])
    want = S.merge(a, b)
    assert S.same(acc.as_dict(), want) is None and want["qualifying"] == 3 + 4 and len(want["hash"]) == 3
    # refusals merge nothing: hashes not strictly ascending, a count of 0; parameters out of range
    for hs, cs in (([3, 3], [1, 1]), ([4, 3], [1, 1]), ([3, 4], [1, 0])):
        with pytest.raises(N.ColordHipError) as e:
            acc.merge(np.array(hs, np.uint64), np.array(cs, np.uint64), 2)
        assert e.value.status == N.CL_E_INVALID and S.same(acc.as_dict(), want) is None
    for size, m in ((0, 2), (2 ** 20 + 1, 2), (5, 0)):
        bad = N.Sketch(size, m)
        with pytest.raises(N.ColordHipError):
            bad.merge(a["hash"], a["count"], 3)
        assert bad.info() == {"size": size, "min_count": m, "qualifying": 0, "n": 0}
    big = N.Sketch(2 ** 20, 1)
    big.merge(a["hash"], a["count"], 3)
    assert big.info()["n"] == 3


# ---- 3. the stream through `info` --------------------------------------------------------------------------------------------------------
def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def stamp(path, payload, name="hipsketch"):
    arc = AR.read_archive(os.path.join(ARC, "bovis24_q_4-avg_balanced.colord"))
    AR.write_archive(path, list(arc.values()) + ([AR.Stream(name, 0, [(0, payload)])] if payload is not None else []))


def printed(o):
    """the sketch of the JSON `info --sketch --json` prints"""
    return {"size": o["size"], "min_count": o["min_count"], "qualifying": o["qualifying"], "hash": np.array(o["hash"], np.uint64), "count": np.array(o["count"], np.uint64)}


def test_hipsketch_round_trip_through_info(tmp_path):
    km = golden_kmers("c1_ont_default")
    arc = str(tmp_path / "s.colord")
    full, whole = S.from_kmers(km, 500, 2), S.from_kmers(km, 10000, 2)
    for s, sets, flags in ((full, 1, 0), (whole, 1, 0), (full, 2, 1)):
        stamp(arc, S.pack(s, 20, 12, sets=sets, flags=flags))
        j = run("info", "--sketch", "--json", arc)
        assert j.returncode == 0, j.stderr
        o = json.loads(j.stdout)
        assert [o[x] for x in ("version", "flags", "k", "f", "min_count", "size", "sets")] == [1, flags, 20, 12, 2, s["size"], sets]
        assert S.same(printed(o), s) is None and o["n"] == len(s["hash"])
        assert all(isinstance(v, int) for v in o["hash"] + o["count"])
        assert "hash sample" in o["note"] and "equal k and f" in o["note"] and "not comparable with Mash" in o["note"]
        complete = len(s["hash"]) < s["size"]
        assert o["complete"] is complete and ("cardinality_estimate" in o) is (not complete)
        t = run("info", "--sketch", arc)
        assert t.returncode == 0, t.stderr
        for text in ("hash sample", "equal k and f", "qualifying: %d\n" % s["qualifying"], "entries: %d\n" % len(s["hash"]), "complete: %s" % ("yes" if complete else "no")):
            assert text in t.stdout, text
        assert ("per set" in t.stdout) is (sets > 1)
        if not complete:
            want = (len(s["hash"]) - 1) * 2.0 ** 64 / int(s["hash"][-1])
            assert abs(o["cardinality_estimate"] - want) <= 1e-12 * want        # a few ulp of a multiply and a divide
            assert "cardinality estimate %.0f beside qualifying %d" % (want, s["qualifying"]) in t.stdout
        i = run("info", arc)
        assert i.returncode == 0 and "k-mer sketch: %d of %d qualifying k-mers" % (len(s["hash"]), s["qualifying"]) in i.stderr
    plain = os.path.join(ARC, "bovis24_q_4-avg_balanced.colord")
    assert "k-mer sketch" not in run("info", plain).stderr
    none = run("info", "--sketch", plain)
    assert none.returncode == 1 and "no k-mer sketch is stored" in none.stderr and none.stdout == ""
    # an empty sketch is one
    stamp(arc, S.pack(S.empty(100, 2), 20, 12))
    o = json.loads(run("info", "--sketch", "--json", arc).stdout)
    assert o["n"] == 0 and o["complete"] is True and o["hash"] == []
    # merged sets: fewer entries than qualifying k-mers in a sketch that is not full is what equal hashes give
    stamp(arc, S.pack(S.from_runs([5, 6, 7], [2, 3, 4], 10, 2), 20, 12, sets=2, qualifying=5))
    o = json.loads(run("info", "--sketch", "--json", arc).stdout)
    assert o["qualifying"] == 5 and o["n"] == 3 and o["sets"] == 2


def _refusals():
    s = S.from_runs([5, 6, 7, 8], [2, 3, 4, 5], 10, 2)
    good = S.pack(s, 20, 12)
    o = np.argsort(s["hash"])
    swapped = dict(s, hash=s["hash"].copy(), count=s["count"].copy())
    swapped["hash"][[1, 2]] = swapped["hash"][[2, 1]]
    equal = dict(s, hash=s["hash"].copy())
    equal["hash"][2] = equal["hash"][1]
    zero = dict(s, count=s["count"].copy())
    zero["count"][3] = 0
    assert list(o) == [0, 1, 2, 3]
    return {"version_2": S.pack(s, 20, 12, version=2), "flags_2": S.pack(s, 20, 12, flags=2), "reserved_1": S.pack(s, 20, 12, reserved=1), "sets_0": S.pack(s, 20, 12, sets=0),
            "n_above_size": S.pack(dict(s, size=3), 20, 12), "incomplete_but_n_is_not_qualifying": S.pack(s, 20, 12, qualifying=5),
            "hashes_descending": S.pack(swapped, 20, 12), "hashes_equal": S.pack(equal, 20, 12), "zero_count": S.pack(zero, 20, 12),
            "one_word_short": good[:-8], "one_byte_more": good + b"\0", "header_only": good[:48], "half_a_header": good[:20],
            "n_says_more": S.pack(s, 20, 12, n=5, qualifying=5), "n_says_fewer": S.pack(s, 20, 12, n=3, qualifying=3)}


@pytest.mark.parametrize("how", sorted(_refusals()))
def test_a_stream_that_is_no_sketch_is_refused_cleanly(how, tmp_path):
    arc, other = str(tmp_path / "s.colord"), str(tmp_path / "o.colord")
    stamp(arc, _refusals()[how])
    stamp(other, S.pack(S.from_runs([5, 6, 7, 8], [2, 3, 4, 5], 10, 2), 20, 12))
    r = run("info", "--sketch", arc)
    assert r.returncode == 1 and "`hipsketch` stream is not one this build reads" in r.stderr and r.stdout == ""
    assert run("info", "--sketch", "--json", arc).returncode == 1
    i = run("info", arc)
    assert i.returncode == 0 and "a `hipsketch` stream this build cannot read" in i.stderr
    for pair in ((arc, other), (other, arc)):
        d = run("dist", *pair)
        assert d.returncode == 1 and d.stdout == "" and arc in d.stderr
    assert run("info", "--sketch", other).returncode == 0


# ---- 4. dist -----------------------------------------------------------------------------------------------------------------------------
def dist_of(tmp_path, a, b, k=20, f=12, ka=None, fa=None, json_out=True, **kw):
    pa, pb = str(tmp_path / "A.colord"), str(tmp_path / "B.colord")
    stamp(pa, S.pack(a, ka or k, fa or f, **kw))
    stamp(pb, S.pack(b, k, f))
    return run("dist", *(["--json"] if json_out else []), pa, pb), pa, pb


def check_dist(o, want):
    for key in ("shared", "compared", "in_a", "in_b"):
        assert o[key] == want[key], (key, o[key], want[key])
    for key in ("jaccard", "containment_of_a", "containment_of_b", "distance"):
        assert abs(o[key] - want[key]) <= 1e-12 * abs(want[key]), (key, o[key], want[key])    # a few ulp of a log and a divide


KEYS = np.arange(1000, 1400, dtype=np.uint64)


def test_dist_of_two_complete_sketches_is_the_exact_jaccard(tmp_path):
    a, b = S.from_runs(KEYS[:60], [2] * 60, 100, 2), S.from_runs(KEYS[40:90], [3] * 50, 100, 2)
    r, pa, pb = dist_of(tmp_path, a, b)
    assert r.returncode == 0, r.stderr
    o = json.loads(r.stdout)
    want = S.dist(a, b, 20)
    assert (want["shared"], want["compared"], want["in_a"], want["in_b"]) == (20, 90, 60, 50) and want["jaccard"] == 20 / 90
    check_dist(o, want)
    assert (o["a"], o["b"], o["k"], o["f"]) == (pa, pb, 20, 12) and r.stderr == ""
    # the text form: one tab-separated line per pair, A against each of the others
    t = run("dist", pa, pb, pa)
    lines = t.stdout.splitlines()
    assert t.returncode == 0 and len(lines) == 2 and lines[0].split("\t")[:2] == [pa, pb] and lines[1].split("\t")[:2] == [pa, pa]
    c = lines[0].split("\t")
    assert len(c) == 8 and (int(c[4]), int(c[5])) == (20, 90) and abs(float(c[2]) - want["distance"]) <= 1e-12 * want["distance"] and abs(float(c[3]) - 20 / 90) <= 1e-15
    assert [float(x) for x in lines[1].split("\t")[2:4]] == [0.0, 1.0]


def test_dist_up_to_the_threshold_both_cover(tmp_path):
    # both full: T is the lower of the two tops and cuts the other sketch strictly inside its range
    a, b = S.from_runs(KEYS[:300], [2] * 300, 50, 2), S.from_runs(KEYS[100:400], [2] * 300, 50, 2)
    ta, tb = int(a["hash"][-1]), int(b["hash"][-1])
    assert ta != tb
    lo, hi = (a, b) if ta < tb else (b, a)
    assert int(hi["hash"][0]) < int(lo["hash"][-1]) < int(hi["hash"][-1])
    want = S.dist(a, b, 20)
    assert 0 < want["shared"] < want["compared"] and min(want["in_a"], want["in_b"]) < 50 == max(want["in_a"], want["in_b"])
    r, _, _ = dist_of(tmp_path, a, b)
    check_dist(json.loads(r.stdout), want)
    # one full, one complete: the full one's top cuts the complete one
    c = S.from_runs(KEYS[:300:7], [2] * len(KEYS[:300:7]), 50, 2)
    assert len(c["hash"]) == 43 and int(c["hash"][0]) < ta < int(c["hash"][-1])
    want = S.dist(a, c, 20)
    assert want["in_a"] == 50 and 0 < want["in_b"] < 43 and want["shared"] == want["in_b"] and want["containment_of_b"] == 1.0
    r, _, _ = dist_of(tmp_path, a, c)
    check_dist(json.loads(r.stdout), want)
    r, _, _ = dist_of(tmp_path, c, a)
    check_dist(json.loads(r.stdout), S.dist(c, a, 20))


def test_dist_at_its_ends(tmp_path):
    a, b = S.from_runs(KEYS[:300], [2] * 300, 50, 2), S.from_runs(KEYS[300:400], [5] * 100, 200, 2)
    o = json.loads(dist_of(tmp_path, a, a)[0].stdout)
    assert (o["jaccard"], o["distance"], o["shared"], o["compared"]) == (1.0, 0.0, 50, 50)
    o = json.loads(dist_of(tmp_path, a, b)[0].stdout)
    assert (o["jaccard"], o["distance"], o["shared"]) == (0.0, 1.0, 0) and o["compared"] == S.dist(a, b, 20)["compared"] > 0
    o = json.loads(dist_of(tmp_path, S.empty(50, 2), S.empty(80, 2))[0].stdout)
    assert (o["compared"], o["shared"], o["jaccard"], o["distance"], o["containment_of_a"], o["containment_of_b"]) == (0, 0, 0.0, 1.0, 0.0, 0.0)


def test_dist_refusals_and_notes(tmp_path):
    a, b = S.from_runs(KEYS[:60], [2] * 60, 100, 2), S.from_runs(KEYS[40:90], [3] * 50, 100, 2)
    for kw in ({"ka": 21}, {"fa": 13}):
        r, pa, pb = dist_of(tmp_path, a, b, **kw)
        assert r.returncode == 1 and r.stdout == "" and "equal k and f" in r.stderr and pa in r.stderr
    m3 = S.from_runs(KEYS[:60], [3] * 60, 100, 3)
    r, pa, pb = dist_of(tmp_path, m3, b)
    assert r.returncode == 0 and "min_count 2, %s with 3" % pa in r.stderr and pb in r.stderr
    check_dist(json.loads(r.stdout), S.dist(m3, b, 20))
    r, pa, pb = dist_of(tmp_path, a, b, sets=2, flags=1)
    assert r.returncode == 0 and "per set" in r.stderr and "reference genome" in r.stderr
    check_dist(json.loads(r.stdout), S.dist(a, b, 20))
    plain = os.path.join(ARC, "bovis24_q_4-avg_balanced.colord")
    r = run("dist", pa, plain)
    assert r.returncode == 1 and r.stdout == "" and "no k-mer sketch is stored" in r.stderr and plain in r.stderr
    r = run("dist", pa, str(tmp_path / "none.colord"))
    assert r.returncode == 1 and "cannot open archive" in r.stderr
    for args in ((pa,), (), ("--nonsense", pa, pb)):
        r = run("dist", *args)
        assert r.returncode == 1 and "usage: colord_hip dist" in r.stderr and r.stdout == ""


# ---- 5. usage ----------------------------------------------------------------------------------------------------------------------------
def test_help_names_the_option():
    r = run("compress-ont", "--help")
    assert r.returncode == 0
    for text in ("--sketch [--sketch-size N] [--sketch-min-count M]", "hipsketch", "HASH SAMPLE", "EQUAL k AND f", "colord_hip info --sketch [--json] archive.colord",
                 "colord_hip dist [--json] A.colord B.colord [C.colord ...]", "10 000 and 2"):
        assert text in r.stderr, text
    r = run("compress-ont", "--sketch", "in.fq")
    assert r.returncode == 1 and "expected input and output paths" in r.stderr and "unknown option" not in r.stderr
    for sub in (["--sketch-size", "500"], ["--sketch-min-count", "3"]):
        r = run("compress-ont", *sub, "in.fq", "out.colord")
        assert r.returncode == 1 and "need --sketch" in r.stderr and "usage" in r.stderr
    for sub in (["--sketch-size", "0"], ["--sketch-size", "1048577"], ["--sketch-min-count", "0"]):
        r = run("compress-ont", "--sketch", *sub, "in.fq", "out.colord")
        assert r.returncode == 1 and "must be in" in r.stderr
    r = run("info", "--sketch", "--kmer-spectrum", "x.colord")
    assert r.returncode == 1 and "usage" in r.stderr
