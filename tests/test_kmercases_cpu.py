"""CPU suite over the constructed read sets of tests/kmercases.py: every case sits on the edge it claims (by kmercases' own model, never by
the code under test), the hash inverse that makes the cases constructible is one, the oracle (oracle/kmer_graph.c) equals the model on
every case and the results the unmodified reference recorded (tests/golden/kmercases/cases.json), and the recorded results belong to
these inputs."""
import numpy as np
import pytest
import kmercases as D
from oracle import pyoracle as O

NAMES = [c["name"] for c in D.CASES]
RECORDED = [c["name"] for c in D.CASES if c["record"] is True]


def test_every_edge_is_held_by_its_cases():
    held = D.check_edges()
    assert len(held) == len(D.EDGES) and all(held.values())
    assert {n for names in held.values() for n in names} == set(NAMES) | set(D.TABLES), "a case that holds no edge"


def test_hash_inverse_round_trips_against_the_oracle():
    rng = np.random.default_rng(1)
    for x in [0, D.M64, 1, 1 << 63, (1 << 56) - 1] + [int(v) for v in rng.integers(0, 1 << 63, 2000)] + [int(v) | (1 << 63) for v in rng.integers(0, 1 << 63, 2000)]:
        h = int(O.lib().orc_hash_mm(x))
        assert D.hash_mm(x) == h and D.hash_inv(h) == x and int(O.lib().orc_hash_mm(D.hash_inv(x))) == x
    v = rng.integers(0, 1 << 63, 1000).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    assert [int(h) for h in D.hash_np(v)] == [D.hash_mm(int(x)) for x in v]


def test_every_case_says_whether_it_is_recorded():
    assert set(D.golden_cases()) == set(RECORDED)
    for c in D.CASES:
        assert c["record"] is True or (isinstance(c["record"], str) and len(c["record"]) > 10), c["name"]
        assert c["record"] is not True or (15 <= c["k"] <= 28 and c["P"] == 0 and D.build(c["name"])["accept"].all())


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_model(name):
    b, m, o = D.build(name), D.model(name), D.oracle_run(name)
    for i, (got, want) in enumerate(zip(o["scan"], m["scan"])):
        assert np.array_equal(got, want[1]), f"scan, read {i}"
    assert np.array_equal(o["keys"], m["kept"]) and np.array_equal(o["counts"], m["kept_counts"]), "kept keys / counts"
    assert o["stats"] == (sum(len(s[1]) for s in m["scan"]), len(m["keys"]), len(m["kept"]), int(m["kept_counts"].sum())), "statistics"
    for i, (got, want) in enumerate(zip(o["lists"], m["lists"])):
        assert np.array_equal(got, want[0]), f"list of read {i}"
    assert o["n_refs"] == m["n_refs"]
    for i in range(b["P"], len(b["reads"])):
        refs, votes, common = o["cands"][i]
        assert (list(refs), list(votes)) == m["cands"][i][:2], f"candidates of read {i}"
        assert [[int(x) for x in cm] for cm in common] == m["cands"][i][2], f"shared k-mers of read {i}"


@pytest.mark.parametrize("name", RECORDED)
def test_recorded_results_belong_to_these_inputs(name):
    import json
    g = D.golden_cases()[name]
    assert g["case"] == {k: v for k, v in json.loads(json.dumps(D.BY_NAME[name])).items() if k != "name"}
    assert g["args"] == D.ref_args(name)
    assert g["input_sha256"] == D.input_sha(name), "the generator drifted: tests/golden/make_kmercases.py"


@pytest.mark.parametrize("name", RECORDED)
def test_oracle_equals_the_reference(name):
    g, o, b = D.golden_cases()[name], D.oracle_run(name), D.build(name)
    p = g["params"]
    assert (p["k"], p["f"], p["ci"], p["cs"], p["c"], p["n_reads"], p["n_pseudo"]) == (b["k"], b["f"], b["ci"], b["cs"], b["c"], len(b["reads"]), 0)
    assert (p["tot_kmers"], p["n_unique"], p["total_count_filtered"]) == (o["stats"][0], o["stats"][2], o["stats"][3])
    assert g["kept"] == {"n": len(o["keys"]), "keys_sha256": D.sha_u(o["keys"], "<u8"), "counts_sha256": D.sha_u(o["counts"], "<u4")}
    lists = [([int(r) for r in refs], [[int(x) for x in cm] for cm in common]) for refs, _, common in o["cands"]]
    if "cands" in g:
        for i, (want, got) in enumerate(zip(g["cands"], lists)):
            assert want == ({"refs": got[0], "common": got[1]} if b["hifi"] else got[0]), f"candidates of read {i}"
        assert len(g["cands"]) == len(lists)
    assert g["cands_sha256"] == D.cands_digest(lists)
