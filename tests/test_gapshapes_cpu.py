"""CPU suite: the constructed gaps of tests/gapshapes.py.  Every case really has the one gap it is meant to have and takes the class and
path the table says (from the oracle's anchors and script and the restated device rules); the oracle's script of the gap equals the
one recorded from the unmodified reference (tests/golden/gapshapes, made by tests/golden/make_gapshapes.py); and the script is in the
bytes the GPU tests compare."""
import hashlib
import json
import os
import numpy as np
import pytest
from oracle import pyoracle as O
import gapshapes as G

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gapshapes")
RECORDED = {r["name"]: r for r in json.load(open(os.path.join(GOLD, "cases.json")))["cases"]}
IDS = [c["name"] for c in G.CASES]


def test_table_is_the_recorded_one():
    assert IDS == list(RECORDED) or sorted(IDS) == sorted(RECORDED), "cases.json is not of this table: run tests/golden/make_gapshapes.py"
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("c", G.CASES, ids=IDS)
def test_generator_has_not_drifted(c):
    r = RECORDED[c["name"]]
    assert {k: (list(v) if isinstance(v, tuple) else v) for k, v in c.items() if k != "name"} == r["case"]
    assert G.seq_sha(c) == r["seq_sha256"]
    p = G.make_parts(c)
    x = np.concatenate([p["Gr"], p["Ge"]])
    raw = np.frombuffer(open(os.path.join(GOLD, "seqs.bin"), "rb").read(), np.uint8, (len(x) + 3) // 4, r["seq_off"])
    bits = np.unpackbits(raw)[:2 * len(x)].reshape(-1, 2)
    assert np.array_equal(bits[:, 0] * 2 + bits[:, 1], x)


@pytest.mark.parametrize("c", G.CASES, ids=IDS)
def test_plan_is_what_the_table_intends(c):
    p = G.plan([c])[0]
    what = G.describe(c, p)
    assert p["anchors"] == G.expected_anchors(c) and p["rev"] == int(c["rc"]), what
    assert (p["nr"], p["ne"]) == (c["nr"], c["ne"]), what
    assert np.array_equal(p["ref_part"], G.make_parts(c)["Gr"]) and np.array_equal(p["enc_part"], G.make_parts(c)["Ge"]), what
    kind = G.GK_TRIVIAL if not (c["nr"] and c["ne"]) else G.GK_INNER if c["where"] == "I" else G.GK_FLANK_TINY if (min(2 * c["ne"], c["nr"]) < 2 or c["ne"] < 2) else G.GK_FLANK
    assert p["kind"] == kind and p["left"] == (c["where"] == "L"), what
    assert (p["rows"], p["cols"]) == G.expected_shape(c), what
    assert p["cls"] == c["cls"] and p["path"] == c["path"], what
    for k in ("dist", "es_len", "sat", "minus1"):
        if k in c:
            assert p[k] == c[k], f"{k}: {what}"
    if p["minus1"]:                                             # pure insertions; the left flank skips the whole reference part first
        assert p["script"] == (b"D" * c["nr"] if c["where"] == "L" else b"") + bytes(b"ACGT"[b] for b in p["enc_part"]) and p["dist"] == c["ne"], what


def test_thresholds_sit_where_the_table_puts_them():
    by = {c["name"]: G.plan([c])[0] for c in G.CASES}
    band = lambda n: G.quad_band(by[n]["kind"], by[n]["rows"], by[n]["cols"])
    assert by["q400_band"]["dist"] == band("q400_band") and by["q400_band1"]["dist"] == band("q400_band1") + 1
    assert by["q400_shw_band"]["dist"] == band("q400_shw_band") == by["q400_shw_band"]["rows"] // 4 + 16
    assert by["q401_shw_band1"]["dist"] == band("q401_shw_band1") + 1 == by["q401_shw_band1"]["rows"] // 4 + 17
    assert G.wave_direct_fits(300, 9709) and not G.wave_direct_fits(300, 9710)
    assert (20 * 6 + 8) * 8192 == 1 << 20 and not G.wave_direct_fits(350, 8192) and G.wave_direct_fits(350, 8191)
    for n, ne in (("w_flank1300_R", 1300), ("w_flank1300_L", 1300), ("w_flank1800_R", 1800), ("w_flank1800_L", 1800)):
        p = by[n]
        assert not G.wave_direct_fits(ne, p["use"]) and p["use"] == 2 * ne
        assert G.wave_direct_fits(ne, p["end1"]) == (ne == 1300) and abs(p["end1"] - ne) <= 8, (n, p["end1"])
    # saturation: entered from rows >= cols + 64 on; the subsequence cases leave rows to the closed form
    assert by["w_rows_cols63"]["rows"] == by["w_rows_cols63"]["cols"] + 63 and by["w_rows_cols64"]["rows"] == by["w_rows_cols64"]["cols"] + 64
    for n in ("w2000x300_subseq", "w5000x300_subseq"):
        assert G.sat_rows(by[n]["ref_part"], by[n]["enc_part"]) % 64 == 0
    # four class-5 gaps share a wave: a last wave with one, two and three gaps, in one call each
    assert {G.totals(G.plan(G.group(g)))[0][5] % 4 for g in G.GROUPS} >= {1, 2, 3}
    assert G.totals(G.plan(G.group("quad")))[1] == 4 and G.totals(G.plan(G.group("giant")))[0][7] == 4


def test_quad_cells_never_decides():
    """gap_class: once rows <= QUAD_ROWS and rows + cols <= QUAD_SEQ hold, the QUAD_CELLS term holds too (largest value 16 x (1087 + 16))"""
    worst = max(((r + 63) // 64) * (G.QUAD_SEQ - r + 16) for r in range(1, G.QUAD_ROWS + 1))
    assert worst == 16 * (1087 + 16) == 17648 < G.QUAD_CELLS


@pytest.mark.parametrize("c", G.CASES, ids=IDS)
def test_oracle_script_equals_the_reference(c):
    r, p = RECORDED[c["name"]], G.plan([c])[0]
    assert (p["es_len"], p["dist"]) == (r["ref_script_len"], r["ref_dist"]), G.describe(c, p)
    assert hashlib.sha256(p["script"]).hexdigest() == r["ref_script_sha256"], G.describe(c, p)


@pytest.mark.parametrize("c", G.CASES, ids=IDS)
def test_script_is_in_the_compared_bytes(c):
    """with every gap accepted (ACCEPT_ALL) the read's tuple stream starts an edit script and spells anchors and the gap's script"""
    ref, read = G.make_pair(c)
    p = G.plan([c])[0]
    enc = O.Encoder(G.A_LEN, G.K_LEN, G.MODULO, 0, **G.ACCEPT_ALL)
    enc.add_ref(ref)
    enc.new_pack()
    t, _ = enc.encode(read, False, [0])
    first, es = G.decode_tuples(t)
    assert first == 10, G.describe(c, p)
    lL, lR = (0 if c["where"] == "L" else c["cores"][0]), (0 if c["where"] == "R" else c["cores"][1])
    script = p["script"]
    if c["where"] == "R":                                       # the trailing deletions of the last fragment are not stored
        script, es = script.rstrip(b"D"), es.rstrip(b"D")
    if len(set(p["enc_part"].tolist())) <= 1 and c["ne"]:        # a constant read part has entropy 0 and is never "cheaper": stored as a literal
        script = bytes(b"ACGT"[b] for b in p["enc_part"]) + (b"D" * c["nr"] if c["where"] != "R" else b"")
    assert es == b"M" * lL + script + b"M" * lR, G.describe(c, p)
