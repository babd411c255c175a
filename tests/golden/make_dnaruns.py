#!/usr/bin/env python3
"""Generates tests/golden/dnaruns/cases.json: for every case of tests/dnaruns.py, at every level of dnaruns.LEVELS, the `dna` stream parts
the UNMODIFIED reference coder makes of the case's tuple streams — oracle/_ref/ref_dna (oracle/ref_harness/ref_dna.cpp: the reference's own
CReferenceReads and CDNACoder, driven as CEntrComprReads drives them) — recorded as [reads, bytes, SHA-256] a part, next to the case's
parameters and the SHA-256 of the case file handed to ref_dna, so that a drift of the generator shows as such.
Only recorded results: the streams are regenerated from their seeds, and nothing of the reference's text or compiled from it is kept.
Run where oracle/_ref/ref_dna is built (make -f oracle/Makefile.ref harness):
    python tests/golden/make_dnaruns.py"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(HERE, "dnaruns")
REF_DNA = os.path.join(ROOT, "oracle", "_ref", "ref_dna")


def main():
    import dnaruns as D
    os.makedirs(OUT, exist_ok=True)
    rec = []
    with tempfile.TemporaryDirectory() as tmp:
        for c in D.CASES:
            levels = {}
            for level in D.LEVELS:
                path = os.path.join(tmp, "case.bin")
                with open(path, "wb") as f:
                    f.write(D.case_file(c["name"], level))
                lines = subprocess.run([REF_DNA, path], check=True, capture_output=True, text=True).stdout.splitlines()
                parts = [[int(x.split()[0]), int(x.split()[1]), x.split()[2]] for x in lines]
                b = D.build(c["name"], level)
                assert [p[0] for p in parts] == [cb[i + 1] - cb[i] for cb in b["calls"] for i in range(len(cb) - 1)]
                levels[str(level)] = {"input_sha256": D.input_sha(c["name"], level), "parts": parts}
            rec.append({"name": c["name"], "case": {k: v for k, v in c.items() if k != "name"}, "levels": levels})
    json.dump({"what": "dna stream parts of constructed tuple streams from the unmodified reference coder (oracle/ref_harness/ref_dna.cpp)", "cases": rec},
              open(os.path.join(OUT, "cases.json"), "w"), indent=0, sort_keys=True)
    print(f"wrote {len(rec)} cases at levels {list(D.LEVELS)}")


if __name__ == "__main__":
    main()
