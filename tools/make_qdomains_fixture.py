#!/usr/bin/env python3
"""Makes the fixture of tests/test_qual_domains_cpu.py — tests/golden/qdomains/reads.fastq.gz and qdomains.colord, an archive whose
quality stream has model domains of its own (`hipqdomains`).  Needs the GPU (the compressor runs there); the test that reads the
fixture does not:

    python tools/make_qdomains_fixture.py

The reads are synthetic (colord_amd.synth, fixed seed) with qualities over a wide alphabet; the archive is what
`colord_hip compress-ont -q org --part-symbols 4096 --qual-domain-symbols 60000 --digest` writes for them."""
import gzip
import os
import subprocess
import sys
import tempfile
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from colord_amd.fastq import write_fastq          # noqa: E402
from colord_amd.synth import make_reads           # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "qdomains")
ARGS = ["compress-ont", "-q", "org", "--part-symbols", "4096", "--qual-domain-symbols", "60000", "--digest"]


def main():
    os.makedirs(OUT, exist_ok=True)
    rs = make_reads(seed=31, genome_len=20_000, target_bases=260_000, mean_scale=1500.0, n_frac=0.2)
    rng = np.random.default_rng(31)
    rs.quals = (33 + np.clip(rng.normal(22, 9, len(rs.quals)), 0, 60).astype(np.uint8)).astype(np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        fq = os.path.join(tmp, "reads.fastq")
        write_fastq(fq, rs)
        raw = open(fq, "rb").read()
        with open(os.path.join(OUT, "reads.fastq.gz"), "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(raw)
        subprocess.check_call([os.path.join(ROOT, "colord_amd", "colord_hip")] + ARGS + [fq, os.path.join(OUT, "qdomains.colord")])
    for n in ("reads.fastq.gz", "qdomains.colord"):
        print(n, os.path.getsize(os.path.join(OUT, n)), "bytes")


if __name__ == "__main__":
    main()
