#!/usr/bin/env python3
"""Generates tests/golden/gapshapes/cases.json and seqs.bin: for every case of tests/gapshapes.py the edit script the UNMODIFIED
reference computes for the case's gap — oracle/_ref/ref_gap (oracle/ref_harness/ref_gap.cpp: the reference's own GetEditDist branches
over its edit_script.h and edlib) — recorded as script length, edit distance, ref_offset and the script's SHA-256, next to the case's
seed and parameters and a SHA-256 of its sequences.  seqs.bin holds the two sides of every gap (reference part, then read part), 2 bits
a symbol, each case from a byte boundary (cases.json: seq_off), so that a drift of the generator shows as such.
Only recorded results: nothing of the reference's text or compiled from it.  Run where oracle/_ref/ref_gap is built:
    python tests/golden/make_gapshapes.py"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(HERE, "gapshapes")
REF_GAP = os.path.join(ROOT, "oracle", "_ref", "ref_gap")


def pack2(x: np.ndarray) -> bytes:
    x = np.asarray(x, np.uint8)
    return np.packbits(np.stack([(x >> 1) & 1, x & 1], axis=1).reshape(-1)).tobytes()


def letters(x) -> str:
    return "".join("ACGT"[b] for b in x) or "-"


def main():
    import gapshapes as G
    os.makedirs(OUT, exist_ok=True)
    parts = [G.make_parts(c) for c in G.CASES]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.txt")
        with open(path, "w") as f:
            for c, p in zip(G.CASES, parts):
                f.write(f"{c['name']} {G.WHERE_CODE[c['where']]}\n{letters(p['Gr'])}\n{letters(p['Ge'])}\n")
        lines = subprocess.run([REF_GAP, path], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(G.CASES)
    blob, rec = bytearray(), []
    for c, p, line in zip(G.CASES, parts, lines):
        name, dist, ref_offset, n, script = line.split()
        script = "" if script == "-" else script
        assert name == c["name"] and int(n) == len(script)
        rec.append({"name": name, "case": {k: (list(v) if isinstance(v, tuple) else v) for k, v in c.items() if k != "name"},
                    "ref_dist": int(dist), "ref_offset": int(ref_offset), "ref_script_len": len(script), "ref_script_sha256": hashlib.sha256(script.encode()).hexdigest(),
                    "seq_sha256": G.seq_sha(c), "seq_off": len(blob)})
        blob += pack2(np.concatenate([p["Gr"], p["Ge"]]))
    json.dump({"what": "edit scripts of constructed gaps from the unmodified reference (oracle/ref_harness/ref_gap.cpp)", "cases": rec}, open(os.path.join(OUT, "cases.json"), "w"), indent=0, sort_keys=True)
    open(os.path.join(OUT, "seqs.bin"), "wb").write(bytes(blob))
    print(f"wrote {len(rec)} cases, {len(blob)} bytes of sequences")


if __name__ == "__main__":
    main()
