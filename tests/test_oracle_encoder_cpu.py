"""CPU suite: oracle encoder (a8-a12: m-mer / k-mer anchors, LIS, gap alignment with edlib's tie-breaking,
static and adaptive cost decisions, recursion into alternative references, tuple emission) against the
tuple streams tapped from the unmodified reference (golden es.bin), fed with the reference's candidates."""
import numpy as np
import pytest
from oracle import pyoracle as O
from util import PLAIN_CONFIGS, golden

# presets (arg_parse.cpp:89-408 / SURVEY App. B): min part length to consider an alternative read, max recursion
PRESET_BY_LEVEL = {1: (64, 3), 2: (48, 5), 3: (48, 6)}


def encode_all(g):
    rs = g.reads
    min_alt, max_rec = PRESET_BY_LEVEL[g.p("level")]
    enc = O.Encoder(g.p("a"), g.p("k"), g.p("f"), g.p("source"), min_part_alt=min_alt, max_rec=max_rec)
    has_n = rs.has_n()
    for i in range(rs.n_reads):
        if g.accept[i] and not has_n[i]:
            enc.add_ref(rs.read(i))
    bounds = rs.pack_bounds()
    out = []
    for pi in range(len(bounds) - 1):
        enc.new_pack()                                     # estimator reset per pack (encoder.cpp:1677)
        for i in range(bounds[pi], bounds[pi + 1]):
            c = g.cands[i]
            out.append(enc.encode(rs.read(i), has_n[i], c["refs"], c["common"] if g.p("source") == 2 else None))
    return out


@pytest.mark.parametrize("cfg", PLAIN_CONFIGS)
def test_tuple_streams_equal_reference(cfg):
    g = golden(cfg)
    got = encode_all(g)
    n_es = 0
    for i, (es, nt) in enumerate(got):
        assert nt == g.es[i][1] and es == g.es[i][2], f"read {i}"
        n_es += es[0] >> 4 == 10
    if cfg in ("c3_clr_ratio", "s6m_ont", "s3m_ont_n_ratio", "s5m_hifi", "c7_hifi_balanced"):
        assert n_es > 10                                    # the edit-script path is really exercised


def test_shw_end_before_target_start():
    """edlib reports end position -1 for SHW when the query length is not a multiple of 64 (edlib.cpp:666-681):
    a flank that shares nothing with the reference is coded as pure insertions, no reference symbol consumed."""
    enc = O.Encoder(16, 20, 12, 0)
    ref = np.array([0] * 40, np.uint8)
    enc.add_ref(ref)
    # reachable through the public entry: a read whose flank shares nothing with its reference (tests/gapshapes.py), and directly
    # through the gap's own entry.  A query of a multiple of 64 symbols has no such end position and consumes reference symbols.
    import gapshapes as G
    cases = [c for c in G.CASES if c["name"].startswith("shw_nothing")]
    assert sorted({c["ne"] for c in cases}) == [63, 64, 65, 128] and {c["where"] for c in cases} == {"L", "R"}
    for c in cases:
        p = G.make_parts(c)
        letters = bytes(b"ACGT"[b] for b in p["Ge"])
        es, dist = O.gap_script(p["Gr"], p["Ge"], G.WHERE_CODE[c["where"]])
        if c["ne"] % 64:
            assert dist == c["ne"] and es == (b"D" * c["nr"] if c["where"] == "L" else b"") + letters, c["name"]
        else:
            assert dist == c["ne"] and sum(es.count(x) for x in b"XYZ") > 0 and not any(x in es for x in b"M"), c["name"]
        ref, read = G.make_pair(c)
        e = O.Encoder(G.A_LEN, G.K_LEN, G.MODULO, 0, **G.ACCEPT_ALL)
        e.add_ref(ref)
        e.new_pack()
        first, whole = G.decode_tuples(e.encode(read, False, [0])[0])
        core = b"M" * (c["cores"][1] if c["where"] == "L" else c["cores"][0])
        assert first == 10 and whole == (es + core if c["where"] == "L" else core + es), c["name"]
