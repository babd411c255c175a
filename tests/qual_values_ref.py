"""The qual-values digest (kind 4) restated in numpy / Python from its definition — the yardstick of
tests/test_qual_values_cpu.py, tests/test_gpu_qual_values.py and tests/test_gpu_cli_digest_values.py.  The values a quality decoder
writes for a read, derived from the INPUT qualities, in two independent forms:

    (a) values_double:  the decoder's own recurrence in IEEE double, `as += avg; v = int(as - qs); qs += v`, fed with the bins of -T and
                        the two average bytes the encoder forms per bin (avg = ((a1 << 8) + a2) / 256)
    (b) values_int:     v_k = floor(k A / 256) - floor((k - 1) A / 256),  k = the 1-based rank of the base among the read's bases of its bin

org: the value itself; *-fix: the -D value of the bin; *-avg: the above per bin; avg: one bin holding every base.  A digest byte is the
value (the decoded ASCII byte - 33); the triple is digest_ref.digest_bytes(kind 4)."""
import struct
import numpy as np
import digest_ref as R

QVAL = 4
FIX, AVG = ("5-fix", "4-fix", "2-fix"), ("5-avg", "4-avg", "2-avg")


def _phred(p):
    """input byte - 33, anything outside 0..95 taken as 0"""
    p = np.asarray(p, np.int64)
    return np.where((p < 0) | (p > 95), 0, p)


def bins_of(mode, phred, T=None):
    """the bin of every base (avg: one bin)"""
    if mode == "avg":
        return np.zeros(len(phred), np.int64)
    return R.map_fwd(mode, T)[phred].astype(np.int64)


def average_A(phred, bins, n_bins):
    """A per bin, as the encoder forms its two average bytes: (uint32)((double)sum / count * 256); 0 for an empty bin"""
    A = []
    for b in range(n_bins):
        sel = phred[bins == b]
        A.append(int(float(int(sel.sum())) / float(len(sel)) * 256) if len(sel) else 0)
    return A


def _n_bins(mode):
    return 1 if mode == "avg" else int(mode[0])


def values_int(mode, phred, T=None, D=None):
    """form (b): integers only.  phred: input byte - 33 of one read.  -> uint8 values"""
    p = _phred(phred)
    if mode == "org":
        return p.astype(np.uint8)
    bins = bins_of(mode, p, T)
    if mode in FIX:
        d = np.asarray(R.DEFAULT_D[mode] if D is None else D, np.int64)
        return d[bins].astype(np.uint8)
    out = np.zeros(len(p), np.uint8)
    for b, A in enumerate(average_A(p, bins, _n_bins(mode))):
        at = np.nonzero(bins == b)[0]
        k = np.arange(1, len(at) + 1, dtype=np.uint64)
        out[at] = ((k * np.uint64(A)) >> np.uint64(8)) - (((k - np.uint64(1)) * np.uint64(A)) >> np.uint64(8))
    return out


def values_double(mode, phred, T=None, D=None):
    """form (a): the decoder's recurrence in double, base by base"""
    p = _phred(phred)
    if mode == "org" or mode in FIX:
        return values_int(mode, p, T, D)
    bins = bins_of(mode, p, T)
    avg = []
    for A in average_A(p, bins, _n_bins(mode)):
        a1, a2 = A >> 8, A & 0xff                                              # the two coded bytes
        avg.append(float((a1 << 8) + a2) / 256.0)
    acc, qs = [0.0] * len(avg), [0.0] * len(avg)
    out = np.zeros(len(p), np.uint8)
    for i, b in enumerate(bins.tolist()):
        acc[b] += avg[b]
        v = int(acc[b] - qs[b])
        qs[b] += v
        out[i] = v
    return out


def digest_values(values, first_read=0):
    """values: per read its uint8 values (decoded ASCII - 33) -> (reads, symbols, sum)"""
    return R.digest_bytes(QVAL, values, first_read)


def digest_input(mode, reads_phred, first_read=0, T=None, D=None):
    return digest_values([values_int(mode, p, T, D) for p in reads_phred], first_read)


def digest_fastq_quality_lines(path, first_read=0):
    """the qual-values digest of the quality lines of a four-line FASTQ"""
    return digest_values([_raw(r[2]) for r in R.parse_fastq(path)], first_read)


def _raw(phred):
    return (np.asarray(phred, np.int64) & 0xff).astype(np.uint8)


def pack_hipdigest2(dna, qual, header, qval):
    """The version-2 `hipdigest` part, 104 bytes: u32 version = 2, u32 flags (bit 3 = qual-values), the triples dna, qual, header, qual-values"""
    flags = (1 if dna else 0) | (2 if qual else 0) | (4 if header else 0) | (8 if qval else 0)
    z = (0, 0, 0)
    return struct.pack("<II12Q", 2, flags, *(dna or z), *(qual or z), *(header or z), *(qval or z))


def unpack_hipdigest_any(b):
    if len(b) == 80:
        return dict(R.unpack_hipdigest(b), qval=None)
    v = struct.unpack("<II12Q", b)
    return dict(version=v[0], flags=v[1], dna=tuple(v[2:5]), qual=tuple(v[5:8]), header=tuple(v[8:11]), qval=tuple(v[11:14]))
