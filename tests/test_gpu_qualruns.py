"""GPU suite over the constructed quality runs of tests/qualruns.py (what each case sits on is asserted there, on the CPU): the quality
coder's parts equal the bytes the unmodified reference coder made (tests/golden/qualruns/cases.json) and the oracle's; after every call
the targeted models (cl_qual_coder_model) equal the oracle's — so a failure says whether the models or the interval coder diverged —
and cl_qual_decode_domains reads the oracle decoder's qualities back from the parts just made.  The group-cut cases run a second time
with COLORD_HIP_QUAL_GROUP_SYMS at the case's size: the same bytes from the number of groups the case claims."""
import hashlib
import numpy as np
import pytest
import torch
import qualruns as Q
from colord_amd.fastq import ReadSet

pytestmark = pytest.mark.gpu
FORMS = [(c["name"], "plain") for c in Q.CASES] + [(c["name"], "group_knob") for c in Q.CASES if "group_syms" in c]


def device_run(ctx, name):
    """(the parts of every call, the targeted models after every call, the groups formed, the domain starts, the decoded qualities)"""
    c, b = Q.BY_NAME[name], Q.build(name)
    fwd, rev = Q._thresholds(c)
    n = b["n_reads"]
    rs = ReadSet(b["bases"], b["off"], b["quals"], [b"r%d" % i for i in range(n)], [False] * n, True)
    reads = ctx.pack_readset(rs)
    qc = ctx.qual_coder(c["mode"], c.get("source", 0), c["level"], fwd, rev)
    try:
        if "domain_symbols" in c:
            qc.set_domain_symbols(Q.domain_symbols_of(name))
        quals = torch.from_numpy(b["quals"]).to(ctx.device)
        qoff = torch.from_numpy(b["off"]).to(ctx.device)
        fl = torch.from_numpy(b["flags"]).to(ctx.device) if c["level"] > 1 else None
        parts, models = [], []
        for cb in b["calls"]:
            out, sizes = qc.encode(reads, quals, qoff, np.asarray(cb), fl)
            raw, o = out.cpu().numpy().tobytes(), 0
            for s in sizes:
                parts.append(raw[o:o + s]); o += s
            models.append({t: qc.model(*t) for t in Q.all_targets(name)})
        groups, doms = qc.groups(), qc.domains()
        payload = torch.from_numpy(np.frombuffer(b"".join(parts), np.uint8).copy()).to(ctx.device)
        decoded = ctx.qual_decode_domains(c["mode"], c.get("source", 0), c["level"], fwd, rev, reads, payload, Q.part_bounds(b), [len(p) for p in parts], doms, qoff, fl)
        return parts, models, groups, doms, decoded.cpu().numpy()
    finally:
        qc.free(); reads.free()


@pytest.mark.parametrize("name,form", FORMS)
def test_parts_equal_reference_models_equal_oracle_and_decode(ctx, name, form, monkeypatch):
    monkeypatch.delenv("COLORD_HIP_QUAL_GROUP_SYMS", raising=False)
    knob = Q.group_syms_of(name) if form == "group_knob" else None
    if knob:
        monkeypatch.setenv("COLORD_HIP_QUAL_GROUP_SYMS", str(knob))
    exp = Q.oracle_run(name)
    parts, models, groups, doms, decoded = device_run(ctx, name)
    for i, (got, want) in enumerate(zip(models, exp["models"])):
        for key in want:
            assert np.array_equal(got[key], want[key]), f"model (family {key[0]}, context {key[1]:#x}) after call {i}: device {got[key].tolist()}, oracle {want[key].tolist()}"
    got = [[len(p), hashlib.sha256(p).hexdigest()] for p in parts]
    assert got == [p[1:] for p in Q.golden_cases()[name]["parts"]], "device parts differ from the reference's"
    assert parts == exp["parts"], "device parts differ from the oracle's"
    assert groups == len(Q.plan(name, knob)), "the call was not cut into the groups the case claims"
    if knob:
        assert groups == Q.BY_NAME[name]["groups"]
    assert doms == Q.domain_starts(name)
    assert np.array_equal(decoded, exp["decoded"]), "cl_qual_decode_domains differs from the oracle's decoder"
