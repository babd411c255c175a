"""CPU suite over the constructed context runs of tests/dnaruns.py: every case has the property it claims (computed by dnaruns' own
model, never by a coder), the recorded results belong to these inputs, the oracle's DNA coder reproduces the parts the unmodified
reference coder made of them (tests/golden/dnaruns/cases.json), and the oracle's models end where the model of dnaruns ends."""
import hashlib
import numpy as np
import pytest
import dnaruns as D

NAMES = [c["name"] for c in D.CASES]


@pytest.mark.parametrize("level", D.LEVELS)
def test_every_edge_is_held_by_its_cases(level):
    held = D.check_edges(level)
    assert len(held) == len(D.EDGES) + len(D.EDGES_EXTRA) + 1
    assert {n for names in held.values() for n in names} == set(NAMES), "a case that holds no edge"


def test_counter_model_in_blocks_equals_one_symbol_at_a_time():
    rng = np.random.default_rng(5)
    for n, mt, ad, L in ((4, 1 << 10, 1, 5000), (8, 1 << 15, 1, 70000), (32, 1 << 18, 8, 70000), (5, 64, 8, 500)):
        syms = rng.choice(n, size=L, p=np.arange(1, n + 1) / (n * (n + 1) / 2))
        a, b = np.ones(n, np.int64), np.ones(n, np.int64)
        assert D.evolve(a, syms, mt, ad) == D.evolve_one_by_one(b, syms, mt, ad) and np.array_equal(a, b)


def test_tuple_writer_round_trips():
    tup = [(D.ANCHOR, 0, (1 << 28) - 1), (D.INS, 3, 0), (D.DEL, 0, 0), (D.MATCH, 0, 0), (D.SUBST, 2, 0), (D.SKIP, 0, 70000), (D.ALT_ID, 0x01020304, 1), (D.MAIN_REF, 0, 0)]
    nt, raw = D.script_read(0xA0B0C0D, 1, tup)
    assert nt == len(tup) + 1 and raw[:5] == bytes([0xA1, 0x0A, 0x0B, 0x0C, 0x0D]) and raw[5:9] == bytes([0x4F, 0xFF, 0xFF, 0xFF])
    assert D.parse_tuples(raw) == [(D.START_ES, 0xA0B0C0D, 1)] + tup
    nt, raw = D.plain_read(np.array([0, 3, 4], np.uint8), True)
    assert nt == 4 and raw == bytes([0xB0, 0x80, 0x83, 0x84])


@pytest.mark.parametrize("level", D.LEVELS)
@pytest.mark.parametrize("name", NAMES)
def test_recorded_results_belong_to_these_inputs(name, level):
    g = D.golden_cases()[name]
    assert g["case"] == {k: v for k, v in _jsonable(D.BY_NAME[name]).items() if k != "name"}
    assert g["levels"][str(level)]["input_sha256"] == D.input_sha(name, level), "the generator drifted: tests/golden/make_dnaruns.py"


def _jsonable(c):
    import json
    return json.loads(json.dumps(c))


@pytest.mark.parametrize("level", D.LEVELS)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_parts_equal_the_reference(name, level):
    got = [[len(p), hashlib.sha256(p).hexdigest()] for p in D.oracle_run(name, level)["parts"]]
    assert got == [p[1:] for p in D.golden_cases()[name]["levels"][str(level)]["parts"]]


@pytest.mark.parametrize("level", D.LEVELS)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_models_end_where_the_model_ends(name, level):
    final = D.oracle_run(name, level)["models"][-1]
    for which, key in enumerate(D.all_targets(name, level)):
        t = D.target(name, level, which)
        assert (t["family"], t["context"]) == key
        assert np.array_equal(final[key], np.append(t["counts"], t["total"])), key
