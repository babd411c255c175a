"""CPU suite over the constructed quality runs of tests/qualruns.py: every case has the property it claims (computed by qualruns' own
model, never by a coder), the recorded results belong to these inputs, the oracle's quality coder reproduces the parts the unmodified
reference coder made of them (tests/golden/qualruns/cases.json), its models end where the model of qualruns ends, and both the oracle's
decoder and the library's host decoder (cl_qual_decode_part) read back the values tests/qual_values_ref.py predicts from the input."""
import ctypes as C
import hashlib
import json
import numpy as np
import pytest
import qualruns as Q

NAMES = [c["name"] for c in Q.CASES]


def test_every_edge_is_held_by_its_cases():
    held = Q.check_edges()
    assert len(held) == len(Q.EDGES) + 5
    assert {n for names in held.values() for n in names} == set(NAMES), "a case that holds no edge"


def test_counter_model_in_blocks_equals_one_symbol_at_a_time():
    rng = np.random.default_rng(5)
    for n, mt, ad, L in ((2, 1 << 10, 8, 3000), (4, 1 << 12, 8, 9000), (5, 64, 8, 500), (96, 1 << 14, 32, 5000), (256, 1 << 13, 8, 6000)):
        syms = rng.choice(n, size=L, p=np.arange(1, n + 1) / (n * (n + 1) / 2))
        a, b = np.ones(n, np.int64), np.ones(n, np.int64)
        assert Q.evolve(a, syms, mt, ad) == Q.evolve_one_by_one(b, syms, mt, ad) and np.array_equal(a, b)


def test_grouping_leaves_the_final_models_alone():
    for name in ("groups_avg4", "groups_avg4_domains"):
        a, b = Q.model_run(name), Q.model_run(name, Q.group_syms_of(name))
        assert a["final"].keys() == b["final"].keys() and all(np.array_equal(a["final"][k], b["final"][k]) for k in a["final"])


@pytest.mark.parametrize("name", NAMES)
def test_recorded_results_belong_to_these_inputs(name):
    g = Q.golden_cases()[name]
    assert g["case"] == {k: v for k, v in json.loads(json.dumps(Q.BY_NAME[name])).items() if k != "name"}
    assert g["input_sha256"] == Q.input_sha(name), "the generator drifted: tests/golden/make_qualruns.py"


@pytest.mark.parametrize("name", NAMES)
def test_oracle_parts_equal_the_reference(name):
    got = [[len(p), hashlib.sha256(p).hexdigest()] for p in Q.oracle_run(name)["parts"]]
    assert got == [p[1:] for p in Q.golden_cases()[name]["parts"]]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_models_end_where_the_model_ends(name):
    final = Q.oracle_run(name)["models"][-1]
    for call, models in enumerate(Q.oracle_run(name)["models"]):
        assert list(models) == Q.all_targets(name)
    for (fam, a), got in final.items():
        want = Q.target_model(name, fam, a)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (f"model (family {fam}, context {a:#x}) after call {len(Q.build(name)['calls']) - 1}: counter {int(bad[0])} "
                              f"(the last is the total) is {int(got[bad[0]])} in the oracle, {int(want[bad[0]])} in the model of qualruns")


@pytest.mark.parametrize("name", NAMES)
def test_oracle_decoder_returns_the_predicted_values(name):
    assert np.array_equal(Q.oracle_run(name)["decoded"], Q.expected_values(name))
    if Q.BY_NAME[name]["mode"] == Q.ORG:
        assert np.array_equal(Q.oracle_run(name)["decoded"], Q.build(name)["quals"])


def host_decode(name, parts):
    """cl_qual_decode_part over the parts, cl_qual_decoder_new_domain at every domain start"""
    from colord_amd import _native as N
    lib = N.load()
    c, b = Q.BY_NAME[name], Q.build(name)
    fwd, rev = Q._thresholds(c)
    prm = N.QualParams(mode=c["mode"], source=c.get("source", 0), level=c["level"], n_fwd=len(fwd), n_rev=len(rev))
    for i, v in enumerate(fwd):
        prm.fwd[i] = v
    for i, v in enumerate(rev):
        prm.rev[i] = v
    q = N._P()
    assert lib.cl_qual_decoder_create(C.byref(prm), C.byref(q)) == 0
    try:
        bases = b["bases"].copy()
        if c["level"] > 1:                                          # the class flags as cl_dna_decode_part hands them on
            bases[b["flags"] == ord("A")] |= 0x80
            bases[b["flags"] == ord("M")] |= 0x40
        o, pb, starts = b["off"], Q.part_bounds(b), Q.domain_starts(name)
        out = np.zeros(len(bases), np.uint8)
        for p, payload in enumerate(parts):
            if p and p in starts:
                assert lib.cl_qual_decoder_new_domain(q) == 0
            r0, r1 = pb[p], pb[p + 1]
            bb = np.ascontiguousarray(bases[o[r0]:o[r1]]); off = (o[r0:r1 + 1] - o[r0]).astype(np.uint64)
            res = np.zeros(max(len(bb), 1), np.uint8); buf = np.frombuffer(payload, np.uint8)
            if not len(bb):
                bb = np.zeros(1, np.uint8)
            assert lib.cl_qual_decode_part(q, buf.ctypes.data, len(buf), bb.ctypes.data, off.ctypes.data, r1 - r0, res.ctypes.data) == 0, (name, p)
            out[o[r0]:o[r1]] = res[:o[r1] - o[r0]]
        return out
    finally:
        lib.cl_qual_decoder_free(q)


@pytest.mark.parametrize("name", NAMES)
def test_host_decoder_returns_the_predicted_values(name):
    assert np.array_equal(host_decode(name, Q.oracle_run(name)["parts"]), Q.expected_values(name))
