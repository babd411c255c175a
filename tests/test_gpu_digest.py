"""GPU suite of the content digest: the kernels of csrc/digest.hip against tests/digest_ref.py (numpy, from the definition) and
against the host quality decoder's digest of what cl_qual_encode wrote; the pipeline's hook (cl_ctx_set_digest); the command line
(`compress-* --digest`, `decompress`, `check`) over every quality mode, the three sequencing modes, FASTA, and the configurations
that cut the input differently (parts, streamed input, domains, ranks), which must all store the same digests.  The shapes are the
smallest at which the kernels can go wrong: every length around a 32-base block and an 8-symbol word, one read that takes a lane
through many strides, more reads than a block holds."""
import ctypes as C
import hashlib
import os
import subprocess
import numpy as np
import pytest
import torch
from colord_amd import _native as N, archive as AR
from colord_amd.fastq import ReadSet, write_fastq
from colord_amd.synth import make_reads
import digest_ref as R
from test_digest_cpu import parse_check

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
REF = os.path.join(ROOT, "oracle", "_ref", "colord")
M64 = (1 << 64) - 1
LENS = [1, 2, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4097, 70_001]
FIRST = [0, 1 << 33]


def sub(a, b):
    return tuple((x - y) & M64 for x, y in zip(a, b))


def edge_readset(seed=3, wide_quals=True):
    """About 40 reads: the edge lengths, N at 0 / 31 / 32 / last, a read of N only, and a few dozen short random reads so that several
    blocks of four waves run; qualities that hit every bin of the default thresholds and the values 0 and 95."""
    rng = np.random.default_rng(seed)
    reads = [rng.integers(0, 4, L).astype(np.uint8) for L in LENS]
    for L, pos in ((33, 0), (64, 31), (65, 32), (2049, 2048), (4097, 0)):
        r = rng.integers(0, 4, L).astype(np.uint8); r[pos] = 4
        reads.append(r)
    reads.append(np.full(40, 4, np.uint8))
    reads += [rng.integers(0, 4, int(L)).astype(np.uint8) for L in rng.integers(1, 300, 22)]
    lens = [len(r) for r in reads]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    q = rng.choice(np.array([0, 3, 6, 7, 10, 13, 14, 20, 25, 26, 40, 92, 93, 95], np.uint8), int(off[-1])) if wide_quals else rng.integers(0, 41, int(off[-1])).astype(np.uint8)
    q[0] = 0; q[-1] = 95
    return ReadSet(np.concatenate(reads), off, (q + 33).astype(np.uint8), [b"r%d" % i for i in range(len(reads))], [False] * len(reads), True), reads


@pytest.fixture(scope="module")
def edge():
    rs, reads = edge_readset()
    phred = [rs.quals[rs.offsets[i]:rs.offsets[i + 1]].astype(np.int64) - 33 for i in range(rs.n_reads)]
    return dict(rs=rs, reads=reads, phred=phred, dna={f: R.digest_bases(reads, f) for f in FIRST})


def pack(ctx, rs, r0=0, r1=None, ascii=False):
    r1 = rs.n_reads if r1 is None else r1
    o = rs.offsets
    codes = rs.bases[o[r0]:o[r1]]
    if ascii:
        codes = np.frombuffer(b"ACGTN", np.uint8)[codes]
    return ctx.pack_reads(torch.from_numpy(np.ascontiguousarray(codes)), torch.from_numpy((o[r0:r1 + 1] - o[r0]).astype(np.int64)), ascii=ascii)


# ---- cl_digest_bases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ascii", [False, True])
@pytest.mark.parametrize("first", FIRST)
def test_bases_equal_the_reference(ctx, edge, ascii, first):
    rs = edge["rs"]
    assert 35 <= rs.n_reads <= 45
    arena = pack(ctx, rs, ascii=ascii)
    assert ctx.digest_bases(arena, first) == edge["dna"][first]
    arena.free()
    # two calls over a split (a cut inside a block of four reads) add up to the one call
    cut = 13
    a, b = pack(ctx, rs, 0, cut, ascii), pack(ctx, rs, cut, None, ascii)
    acc = N.Digest()
    ctx.digest_bases(b, first + cut, acc)
    assert ctx.digest_bases(a, first, acc) == edge["dna"][first]
    a.free(); b.free()


def test_bases_read_by_read(ctx, edge):
    """Each read alone, at its index: a wrong term cannot hide behind another (and a launch of one wave)."""
    rs, reads = edge["rs"], edge["reads"]
    for i in list(range(19)):
        arena = pack(ctx, rs, i, i + 1)
        assert ctx.digest_bases(arena, i) == R.digest_bases([reads[i]], i), (i, len(reads[i]))
        arena.free()


def test_read_index_range_is_checked(ctx, edge):
    arena = pack(ctx, edge["rs"], 0, 2)
    with pytest.raises(N.ColordHipError, match="2\\^63"):
        ctx.digest_bases(arena, (1 << 63) - 1)
    assert ctx.digest_bases(arena, (1 << 63) - 2)[0] == 2
    arena.free()


# ---- cl_digest_quals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["org", "5-fix", "4-fix", "2-fix"])
def test_quals_of_the_per_base_modes_equal_the_reference(ctx, edge, mode):
    rs = edge["rs"]
    arena = pack(ctx, rs)
    quals, qoff = torch.from_numpy(rs.quals).to(ctx.device), torch.from_numpy(rs.offsets).to(ctx.device)
    for first in FIRST:
        assert ctx.digest_quals(arena, quals, qoff, R.QUAL_MODES.index(mode), R.DEFAULT_T.get(mode, ()), first) == R.digest_quals_fixed(mode, edge["phred"], first)
    # other thresholds (a bin that is empty, a bin from 0); a split into two calls with offsets that do not start at 0
    if mode == "4-fix":
        t = [0, 14, 95]
        assert ctx.digest_quals(arena, quals, qoff, 5, t, 7) == R.digest_quals_fixed(mode, edge["phred"], 7, t)
    cut = 14
    a, b = pack(ctx, rs, 0, cut), pack(ctx, rs, cut)
    acc = N.Digest()
    ctx.digest_quals(b, quals, qoff[cut:], R.QUAL_MODES.index(mode), R.DEFAULT_T.get(mode, ()), 5 + cut, acc)       # (the quality offsets of a later chunk: any alignment)
    assert ctx.digest_quals(a, quals, qoff[:cut + 1], R.QUAL_MODES.index(mode), R.DEFAULT_T.get(mode, ()), 5, acc) == R.digest_quals_fixed(mode, edge["phred"], 5)
    arena.free(); a.free(); b.free()


def host_decoder_digest(rs, parts, bounds, mode, source, rev, first):
    """The qual digest the host quality decoder reports after decoding `parts` (level 1: the bases carry no flags)."""
    lib = N.load()
    prm = N.QualParams(mode=mode, source=source, level=1, n_fwd=0, n_rev=len(rev))
    for i, v in enumerate(rev):
        prm.rev[i] = v
    q = N._P()
    assert lib.cl_qual_decoder_create(C.byref(prm), C.byref(q)) == 0
    assert lib.cl_qual_decoder_set_digest(q, 1, first) == 0
    o = rs.offsets
    for p, payload in enumerate(parts):
        r0, r1 = int(bounds[p]), int(bounds[p + 1])
        bases = np.ascontiguousarray(rs.bases[o[r0]:o[r1]]); off = (o[r0:r1 + 1] - o[r0]).astype(np.uint64)
        out = np.zeros(max(len(bases), 1), np.uint8); buf = np.frombuffer(payload, np.uint8)
        assert lib.cl_qual_decode_part(q, buf.ctypes.data, len(buf), bases.ctypes.data, off.ctypes.data, r1 - r0, out.ctypes.data) == 0
    d = N.Digest()
    assert lib.cl_qual_decoder_digest(q, C.byref(d)) == 0
    lib.cl_qual_decoder_free(q)
    return d.triple()


@pytest.fixture(scope="module")
def few_hundred():
    """A few hundred reads: the edge reads (qualities 0..40, every bin) and random ones."""
    rs, _ = edge_readset(seed=5, wide_quals=False)
    more = make_reads(seed=9, genome_len=20_000, target_bases=150_000, mean_scale=500.0)
    rng = np.random.default_rng(2)
    mq = (33 + np.clip(rng.normal(18, 11, len(more.quals)), 0, 93).astype(np.uint8)).astype(np.uint8)
    off = np.concatenate([rs.offsets, rs.offsets[-1] + more.offsets[1:]]).astype(np.int64)
    n = len(off) - 1
    return ReadSet(np.concatenate([rs.bases, more.bases]), off, np.concatenate([rs.quals, mq]), [b"r%d" % i for i in range(n)], [False] * n, True)


@pytest.mark.parametrize("mode", list(range(9)), ids=R.QUAL_MODES)
def test_quals_of_every_mode_equal_the_decoders_digest(ctx, few_hundred, mode):
    """For all nine modes and the three sources: the device digest of the input's quality symbols is what the host decoder digests while it decodes
    the parts cl_qual_encode wrote for the same reads (one part; three parts).  Mode none: nothing is coded, nothing digested."""
    from oracle import pyoracle as O
    from test_gpu_qual import gpu_encode
    rs = few_hundred
    assert 200 <= rs.n_reads <= 900
    n = rs.n_reads
    fwd, rev = O.QUAL_DEFAULTS[mode]
    arena = pack(ctx, rs)
    quals, qoff = torch.from_numpy(rs.quals).to(ctx.device), torch.from_numpy(rs.offsets).to(ctx.device)
    first = 1 << 33
    dev = ctx.digest_quals(arena, quals, qoff, mode, fwd, first)
    arena.free()
    if mode == 8:
        assert dev == (0, 0, 0)
    else:
        navg = {1: 10, 2: 8, 3: 4, 7: 2}.get(mode, 0)
        assert dev[:2] == (n, navg * n + (int(rs.offsets[-1]) if mode != 7 else 0))
    for source in (0, 1, 2):
        for bounds in (np.array([0, n], np.int64), np.array([0, n // 3, n // 2, n], np.int64)):
            parts = gpu_encode(ctx, rs, mode, source, 1, bounds) if mode != 8 else [b""] * (len(bounds) - 1)
            assert host_decoder_digest(rs, parts, bounds, mode, source, rev, first) == dev, (source, len(bounds))


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------------
def test_drivers_digest_their_input_and_only_when_asked():
    """cl_ctx_set_digest: the one-call driver and the chunked compressor add the digests of their reads (global indices over the chunks) to the
    context's totals and write the parts they write without it; off (the default): zeroes, and no digest kernel in a timed context's table."""
    from util import golden
    from bench import reference_part_bounds
    from oracle import pyoracle as O
    from colord_amd.device import Context
    from test_gpu_stream import params_of, one_call, chunked, even_cuts
    g = golden("s6m_ont")
    rs, prm = g.reads, params_of(g)
    packs = reference_part_bounds(np.diff(rs.offsets).astype(np.uint32), 1 << 19)
    qm = g.p("qual_mode"); d = O.QUAL_DEFAULTS[qm]
    qual_args = (qm, g.p("source"), g.p("level"), tuple(d[0]), tuple(d[1]))
    c = Context(0, timing=True)
    try:
        off_one = one_call(c, rs, prm, packs, qual_args)
        assert c.digest() == ((0, 0, 0), (0, 0, 0))
        assert not [k for k in c.kernel_times() if "digest" in k] and not [k for k in c.acc if "digest" in k]
        c.set_digest(True)
        on_one = one_call(c, rs, prm, packs, qual_args)
        d1 = c.digest()
        names = set(c.kernel_times()) | set(c.acc)
        assert {"k_digest_bases", "k_digest_quals"} <= names
        on_chunked = chunked(c, rs, prm, packs, even_cuts(len(packs) - 1, 3), qual_args, announce="all")
        d2 = c.digest()
        c.set_digest(False)
        one_call(c, rs, prm, packs, qual_args)
        assert c.digest() == d2
    finally:
        c.close()
    assert on_one[:4] == off_one[:4] and on_chunked[:4] == off_one[:4]
    reads = [rs.bases[rs.offsets[i]:rs.offsets[i + 1]] for i in range(rs.n_reads)]
    assert d1[0] == R.digest_bases(reads) and sub(d2[0], d1[0]) == d1[0]
    navg = {1: 10, 2: 8, 3: 4}.get(qm, 0)                                      # (the *-avg modes code 2 x bins average bytes in front of a read's bases)
    assert qm <= 6 and d1[1][:2] == (rs.n_reads, navg * rs.n_reads + int(rs.offsets[-1])) and sub(d2[1], d1[1]) == d1[1]


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def _streams(path):
    return {name: [(m, hashlib.sha256(p).hexdigest()) for m, p in s.parts] for name, s in AR.read_archive(path).items() if name != "info"}


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """2 Mbases of the project's generator as FASTQ and FASTA, with a few '+' lines that repeat the id and a read with N."""
    d = tmp_path_factory.mktemp("digest_in")
    rs = make_reads(seed=21, genome_len=100_000, target_bases=2_000_000, mean_scale=5000.0, n_frac=0.0005)
    rs.plus_eq = [i % 7 == 0 for i in range(rs.n_reads)]
    fq, fa = str(d / "in.fastq"), str(d / "in.fasta")
    write_fastq(fq, rs)
    lut = np.frombuffer(b"ACGTN", np.uint8)
    with open(fa, "wb") as f:
        for i in range(rs.n_reads):
            f.write(b">" + rs.headers[i] + b"\n" + lut[rs.bases[rs.offsets[i]:rs.offsets[i + 1]]].tobytes() + b"\n")
    reads = [rs.bases[rs.offsets[i]:rs.offsets[i + 1]] for i in range(rs.n_reads)]
    return dict(fq=fq, fa=fa, rs=rs, dna=R.digest_bases(reads),
                header=R.digest_bytes(R.HEADER, [R.header_bytes(rs.headers[i], rs.plus_eq[i]) for i in range(rs.n_reads)]),
                header_fasta=R.digest_bytes(R.HEADER, [R.header_bytes(h, False) for h in rs.headers]))


def stored_digest(path):
    arc = AR.read_archive(path)
    assert "hipdigest" in arc and len(arc["hipdigest"].parts) == 1
    meta, payload = arc["hipdigest"].parts[0]
    assert meta == 0 and len(payload) == 80
    return R.unpack_hipdigest(payload)


CLI_CASES = [("compress-ont", ["-q", m], "fq") for m in R.QUAL_MODES] + [("compress-pbhifi", [], "fq"), ("compress-pbraw", [], "fq"), ("compress-ont", [], "fa")]


@pytest.mark.parametrize("mode,extra,kind", CLI_CASES, ids=[f"{m}{'_' + e[1] if e else ''}_{k}" for m, e, k in CLI_CASES])
def test_cli_digest_archive(tmp_path, synth, mode, extra, kind):
    src = synth[kind]
    plain, dig, out = str(tmp_path / "off.colord"), str(tmp_path / "on.colord"), str(tmp_path / "o.fastq")
    subprocess.check_call([CLI, mode] + extra + [src, plain], stderr=subprocess.DEVNULL)
    subprocess.check_call([CLI, mode, "--digest"] + extra + [src, dig], stderr=subprocess.DEVNULL)
    a, b = _streams(plain), _streams(dig)
    assert "hipdigest" not in a and set(b) == set(a) | {"hipdigest"}
    assert {k: v for k, v in b.items() if k != "hipdigest"} == a                # every other stream but `info`: the bytes of the run without the option
    st = stored_digest(dig)
    qual_mode = extra[1] if extra else {"compress-ont": "4-avg", "compress-pbhifi": "5-avg", "compress-pbraw": "none"}[mode]
    has_qual = kind == "fq" and qual_mode != "none"
    assert st["version"] == 1 and st["flags"] == (7 if has_qual else 5)
    assert st["dna"] == synth["dna"] and st["header"] == (synth["header"] if kind == "fq" else synth["header_fasta"])
    if not has_qual:
        assert st["qual"] == (0, 0, 0)
    elif qual_mode in ("org", "5-fix", "4-fix", "2-fix"):
        rs = synth["rs"]
        assert st["qual"] == R.digest_quals_fixed(qual_mode, [rs.quals[rs.offsets[i]:rs.offsets[i + 1]].astype(np.int64) - 33 for i in range(rs.n_reads)])
    r = subprocess.run([CLI, "decompress", dig, out], capture_output=True, text=True)
    names = "dna, qual, header" if has_qual else "dna, header"
    assert r.returncode == 0 and f"content digest: ok ({names})" in r.stderr, r.stderr
    c = subprocess.run([CLI, "check", dig], capture_output=True, text=True)
    assert c.returncode == 0, c.stdout + c.stderr
    got = parse_check(c.stdout)
    for k in ("dna", "header") + (("qual",) if has_qual else ()):
        assert got[k] == st[k] == got["stored " + k]
    r2 = subprocess.run([CLI, "decompress", plain, str(tmp_path / "p.fastq")], capture_output=True, text=True)
    assert r2.returncode == 0 and "content digest" not in r2.stderr and sha(out) == sha(str(tmp_path / "p.fastq"))


@pytest.fixture(scope="module")
def baseline_digest(tmp_path_factory, synth):
    arc = str(tmp_path_factory.mktemp("digest_base") / "base.colord")
    subprocess.check_call([CLI, "compress-ont", "--digest", synth["fq"], arc], stderr=subprocess.DEVNULL)
    return stored_digest(arc)


@pytest.mark.parametrize("extra", [["--part-symbols", "65536"], ["--stream-input", "--chunk-bases", "5e5"], ["--domains", "2"], ["--gpus", "2", "--gpu-list", "0,0", "--transport", "host"],
                                   ["--chunk-bases", "3e5"]], ids=["part_symbols", "stream_input", "domains", "two_ranks", "chunks"])
def test_cli_digest_is_the_same_however_the_input_is_cut(tmp_path, synth, baseline_digest, extra):
    arc, out = str(tmp_path / "x.colord"), str(tmp_path / "o.fastq")
    subprocess.check_call([CLI, "compress-ont", "--digest"] + extra + [synth["fq"], arc], stderr=subprocess.DEVNULL)
    assert stored_digest(arc) == baseline_digest
    r = subprocess.run([CLI, "decompress", arc, out], capture_output=True, text=True)
    assert r.returncode == 0 and "content digest: ok (dna, qual, header)" in r.stderr, r.stderr


def test_reference_decompressor_ignores_the_digest_stream(tmp_path, synth):
    assert os.path.exists(REF), "oracle/_ref/colord is built by build()"
    plain, dig = str(tmp_path / "off.colord"), str(tmp_path / "on.colord")
    subprocess.check_call([CLI, "compress-ont", synth["fq"], plain], stderr=subprocess.DEVNULL)
    subprocess.check_call([CLI, "compress-ont", "--digest", synth["fq"], dig], stderr=subprocess.DEVNULL)
    for arc, out in ((plain, "p.fastq"), (dig, "d.fastq")):
        subprocess.check_call([REF, "decompress", arc, str(tmp_path / out)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert sha(str(tmp_path / "p.fastq")) == sha(str(tmp_path / "d.fastq"))
