#!/usr/bin/env python3
"""Generates tests/golden/kmercases/cases.json: for every case of tests/kmercases.py that the reference's command line can express
(k from 15 to 28, no pseudo reads, every read without N a reference read, a counted k-mer set) what the UNMODIFIED reference makes of it —
oracle/_ref/ref_dump (oracle/ref_harness/ref_dump.cpp: the reference's own stages with taps on their queues), run on the case written as
FASTQ with `compress-ont` (HiFi cases: `compress-pbhifi`) `-k -L -H -f -c`.  Per case: the parameters of params.txt, the SHA-256 of the
FASTQ handed over (a drift of the generator shows as such), number and SHA-256 of the kept k-mers and of their counts, and the candidate
lists (with the shared k-mers of HiFi cases): in full where small, always as a digest.
Only recorded results: the reads are regenerated from their seeds, and nothing of the reference's text or compiled from it is kept.
Run where oracle/_ref/ref_dump is built (make -C oracle ref):
    python tests/golden/make_kmercases.py"""
import json
import os
import struct
import subprocess
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(HERE, "kmercases")
REF_DUMP = os.path.join(ROOT, "oracle", "_ref", "ref_dump")
PARAMS = ("k", "f", "ci", "cs", "c", "source", "sparse", "n_reads", "tot_kmers", "n_unique", "total_count_filtered", "n_pseudo")
FULL_LISTS_UP_TO = 300                                    # candidate entries (and shared k-mers) stored in full


def parse_cands(raw: bytes):
    p, out = 0, []
    while p < len(raw):
        rid, has_n, ln, n = struct.unpack_from("<IBII", raw, p); p += 13
        refs = list(struct.unpack_from("<%dI" % n, raw, p)); p += 4 * n
        common = []
        for _ in range(n):
            (m,) = struct.unpack_from("<I", raw, p); p += 4
            common.append([int(x) for x in np.frombuffer(raw, "<u8", m, p)]); p += 8 * m
        out.append((rid, refs, common))
    out.sort(key=lambda e: e[0])
    return out


def main():
    import kmercases as D
    os.makedirs(OUT, exist_ok=True)
    rec = []
    for c in D.CASES:
        if c["record"] is not True:
            print(f"{c['name']}: oracle-only ({c['record']})")
            continue
        with tempfile.TemporaryDirectory() as tmp:
            inp, dump = os.path.join(tmp, "case.fastq"), os.path.join(tmp, "dump")
            with open(inp, "wb") as f:
                f.write(D.fastq_bytes(c["name"]))
            r = subprocess.run([REF_DUMP] + D.ref_args(c["name"]) + ["-t", "4", inp, os.path.join(tmp, "out.colord")],
                               env=dict(os.environ, COLORD_DUMP_DIR=dump), capture_output=True, text=True)
            if r.returncode:
                raise SystemExit(f"{c['name']}: the reference ended with {r.returncode}\n{r.stderr[-2000:]}\n"
                                 "(a case the reference refuses is marked oracle-only in tests/kmercases.py, with the reason)")
            params = {}
            for line in open(os.path.join(dump, "params.txt")):
                key, v = line.split()
                if key in PARAMS:
                    params[key] = int(v)
            b = D.build(c["name"])
            assert (params["k"], params["f"], params["ci"], params["cs"], params["c"]) == (c["k"], c["f"], c["ci"], c["cs"], c["c"]), params
            assert params["n_reads"] == len(b["reads"]) and params["n_pseudo"] == 0
            accept = np.fromfile(os.path.join(dump, "accept.bin"), np.uint8)
            assert accept.all() and len(accept) == len(b["reads"]), f"{c['name']}: the reference does not accept every read"
            kept = np.fromfile(os.path.join(dump, "kept.bin"), np.dtype([("k", "<u8"), ("c", "<u4")]))
            o = np.argsort(kept["k"], kind="stable")
            cands = parse_cands(open(os.path.join(dump, "cands.bin"), "rb").read())
            assert [e[0] for e in cands] == list(range(len(b["reads"])))
            lists = [(e[1], e[2] if c["hifi"] else []) for e in cands]
            entry = {"name": c["name"], "case": {k: v for k, v in c.items() if k != "name"}, "args": D.ref_args(c["name"]), "params": params,
                     "input_sha256": D.input_sha(c["name"]),
                     "kept": {"n": int(len(kept)), "keys_sha256": D.sha_u(kept["k"][o], "<u8"), "counts_sha256": D.sha_u(kept["c"][o], "<u4")},
                     "cands_sha256": D.cands_digest(lists)}
            if sum(len(r_) + sum(len(x) for x in cm) for r_, cm in lists) <= FULL_LISTS_UP_TO:
                entry["cands"] = [{"refs": r_, "common": cm} if c["hifi"] else r_ for r_, cm in lists]
            rec.append(entry)
            print(c["name"], params["tot_kmers"], len(kept), sum(len(r_) for r_, _ in lists))
    json.dump({"what": "kept k-mers and candidate lists of constructed read sets from the unmodified reference (oracle/ref_harness/ref_dump.cpp)",
               "cases": rec}, open(os.path.join(OUT, "cases.json"), "w"), indent=0, sort_keys=True)
    print(f"wrote {len(rec)} cases")


if __name__ == "__main__":
    main()
