#!/usr/bin/env python3
"""Generates tests/golden/qualruns/cases.json: for every case of tests/qualruns.py the `qual` stream parts the UNMODIFIED reference coder
makes of the case's reads — oracle/_ref/ref_qual (oracle/ref_harness/ref_qual.cpp: the reference's own CQualityCoder, driven as
CEntrComprQuals drives it) — recorded as [reads, bytes, SHA-256] a part, next to the case's parameters and the SHA-256 of the case file
handed to ref_qual, so that a drift of the generator shows as such.  A case with model domains, which the reference does not have, is
handed over a domain at a time: a domain is coded as by a fresh coder.
Only recorded results: the reads are regenerated from their seeds, and nothing of the reference's text or compiled from it is kept.
Run where oracle/_ref/ref_qual is built (make -f oracle/Makefile.ref harness):
    python tests/golden/make_qualruns.py"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(HERE, "qualruns")
REF_QUAL = os.path.join(ROOT, "oracle", "_ref", "ref_qual")


def main():
    import qualruns as Q
    os.makedirs(OUT, exist_ok=True)
    rec = []
    with tempfile.TemporaryDirectory() as tmp:
        for c in Q.CASES:
            parts = []
            for p0, p1 in Q.domain_reads(c["name"]):
                path = os.path.join(tmp, "case.bin")
                with open(path, "wb") as f:
                    f.write(Q.case_file(c["name"], p0, p1))
                lines = subprocess.run([REF_QUAL, path], check=True, capture_output=True, text=True).stdout.splitlines()
                parts += [[int(x.split()[0]), int(x.split()[1]), x.split()[2]] for x in lines]
            pb = Q.part_bounds(Q.build(c["name"]))
            assert [p[0] for p in parts] == [b - a for a, b in zip(pb, pb[1:])]
            rec.append({"name": c["name"], "case": {k: v for k, v in c.items() if k != "name"}, "input_sha256": Q.input_sha(c["name"]), "parts": parts})
    json.dump({"what": "qual stream parts of constructed read sets from the unmodified reference coder (oracle/ref_harness/ref_qual.cpp)", "cases": rec},
              open(os.path.join(OUT, "cases.json"), "w"), indent=0, sort_keys=True)
    print(f"wrote {len(rec)} cases")


if __name__ == "__main__":
    main()
