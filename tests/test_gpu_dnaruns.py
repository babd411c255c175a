"""GPU suite over the constructed context runs of tests/dnaruns.py (what each case sits on is asserted there, on the CPU): the DNA
coder's parts equal the bytes the unmodified reference coder made (tests/golden/dnaruns/cases.json) and the oracle's, and after every
call the targeted models (cl_dna_coder_model) equal the oracle's — so a failure says whether the models or the interval coder diverged.
Every case at level 1 with 32-bit keys, at level 1 with 64-bit keys (COLORD_HIP_DNA_WIDE_KEYS) and at level 3; with COLORD_HIP_LONG_RUN
unset, so that the run is evolved by k_dna_evolve, and set to the case's threshold, so that it goes through k_long_*."""
import hashlib
import numpy as np
import pytest
import torch
import dnaruns as D
from colord_amd.fastq import ReadSet

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in D.CASES]
FORMS = {"level1": (1, False), "level1_wide_keys": (1, True), "level3": (3, False)}


def device_run(ctx, name, level):
    """(the parts of every call, the targeted models after every call) from the device coder"""
    b = D.build(name, level)
    lens = np.array([len(r) for r in b["refs"]], np.int64)
    refs = ctx.pack_readset(ReadSet(np.concatenate(b["refs"]).astype(np.uint8), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), None, [], [], False))
    dc = ctx.dna_coder(b["max_alt"], level, D.START_READ_ID)
    parts, models = [], []
    try:
        for cb in b["calls"]:
            reads = b["reads"][cb[0]:cb[-1]]
            raw = b"".join(r[1] for r in reads)
            es = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(ctx.device)
            off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r[1]) for r in reads])]).astype(np.int64)).to(ctx.device)
            nt = torch.from_numpy(np.array([r[0] for r in reads], np.int32)).to(ctx.device)
            out, sizes = dc.encode(refs, es, off, nt, np.asarray(cb) - cb[0])
            out, o = out.cpu().numpy().tobytes(), 0
            for s in sizes:
                parts.append(out[o:o + s]); o += s
            models.append({(f, x): dc.model(D.FAM[f], x) for f, x in D.all_targets(name, level)})
    finally:
        dc.free(); refs.free()
    return parts, models


@pytest.mark.parametrize("path", ["short_path", "long_path"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", NAMES)
def test_parts_equal_reference_and_models_equal_oracle(ctx, name, form, path, monkeypatch):
    level, wide = FORMS[form]
    c = D.BY_NAME[name]
    for k in ("COLORD_HIP_LONG_RUN", "COLORD_HIP_DNA_WIDE_KEYS", "COLORD_HIP_WALK_CHUNK", "COLORD_HIP_WALK_WARM"):
        monkeypatch.delenv(k, raising=False)
    if path == "long_path":
        monkeypatch.setenv("COLORD_HIP_LONG_RUN", str(c["long_run"]))
    if wide:
        monkeypatch.setenv("COLORD_HIP_DNA_WIDE_KEYS", "1")
    if "walk_chunk" in c:
        monkeypatch.setenv("COLORD_HIP_WALK_CHUNK", str(c["walk_chunk"]))
    exp = D.oracle_run(name, level)
    parts, models = device_run(ctx, name, level)
    for i, (got, want) in enumerate(zip(models, exp["models"])):
        for key in want:
            assert np.array_equal(got[key], want[key]), f"model {key} after call {i}: device {got[key].tolist()}, oracle {want[key].tolist()}"
    got = [[len(p), hashlib.sha256(p).hexdigest()] for p in parts]
    assert got == [p[1:] for p in D.golden_cases()[name]["levels"][str(level)]["parts"]], "device parts differ from the reference's"
    assert parts == exp["parts"], "device parts differ from the oracle's"
