"""ctypes binding of libcolord_hip.so (the C ABI in include/colord_hip.h).

There is deliberately NO fallback: if the shared library is missing or a call fails, an exception is
raised.  Device memory is supplied by the caller (torch CUDA tensors -> data_ptr()).
"""
from __future__ import annotations
import ctypes as C
import os

# more hardware queues than the HIP runtime's default of 4: the contexts of one compressor keep up to ten streams busy and
# streams that share a queue serialise (bench.py has the measurement); only effective before the runtime initialises
os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("COLORD_HIP_LIBRARY") or os.path.join(_HERE, "libcolord_hip.so")    # (COLORD_HIP_LIBRARY: another build of the same library, for A/B measurements)

CL_OK, CL_E_INVALID, CL_E_HIP, CL_E_CAPACITY, CL_E_NOMEM, CL_E_UNSUPPORTED, CL_E_MISMATCH = 0, -1, -2, -3, -4, -5, -6


class ColordHipError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"colord_hip error {status}: {msg}")
        self.status = status


class QualParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("source", C.c_int32), ("level", C.c_int32), ("n_fwd", C.c_uint32), ("fwd", C.c_uint32 * 8),
                ("n_rev", C.c_uint32), ("rev", C.c_uint32 * 8)]


class KmerStats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("tot_kmers", C.c_uint64), ("n_unique", C.c_uint64),
                ("n_unique_counted", C.c_uint64), ("total_count_filtered", C.c_uint64)]


class Digest(C.Structure):
    """cl_digest: reads and symbols counted, and the 64-bit content sum; digests of disjoint sets of reads add field by field."""
    _fields_ = [("reads", C.c_uint64), ("symbols", C.c_uint64), ("sum", C.c_uint64)]

    def triple(self):
        return self.reads, self.symbols, self.sum


class Report(C.Structure):
    """cl_report: the content report; every field adds over disjoint sets of reads except len_min / len_max (min / max) and has_qual (or)."""
    _fields_ = [("reads", C.c_uint64), ("bases", C.c_uint64), ("base_count", C.c_uint64 * 5), ("len_min", C.c_uint64), ("len_max", C.c_uint64),
                ("len_hist", C.c_uint64 * 33), ("len_bases", C.c_uint64 * 33), ("has_qual", C.c_uint64), ("q_reads", C.c_uint64), ("q_symbols", C.c_uint64),
                ("mean_q_hist", C.c_uint64 * 96), ("q_joint", (C.c_uint64 * 96) * 96)]

    def as_dict(self):
        """plain ints and numpy arrays, field by field"""
        import numpy as np
        out = {}
        for name, t in self._fields_:
            v = getattr(self, name)
            out[name] = int(v) if t is C.c_uint64 else np.ctypeslib.as_array(v).copy()
        return out


class Edits(C.Structure):
    """cl_edits: the edit-operation profile; every field is an unsigned 64-bit counter that adds over disjoint sets of reads."""
    _fields_ = [("reads", C.c_uint64), ("bases", C.c_uint64), ("kind_reads", C.c_uint64 * 3), ("kind_bases", C.c_uint64 * 3), ("kind_bytes", C.c_uint64 * 3),
                ("main_rev", C.c_uint64 * 2), ("tuples", C.c_uint64 * 8), ("anchor_bases", C.c_uint64), ("anchor_len_hist", C.c_uint64 * 29),
                ("skip_entries", C.c_uint64), ("skip_entry_sum", C.c_uint64), ("skip_bases", C.c_uint64), ("skip_len_hist", C.c_uint64 * 29),
                ("ins_base", C.c_uint64 * 4), ("del_base", C.c_uint64 * 4), ("match_base", C.c_uint64 * 4), ("sub", (C.c_uint64 * 4) * 4),
                ("ins_run_hist", C.c_uint64 * 17), ("del_run_hist", C.c_uint64 * 17), ("identity_hist", C.c_uint64 * 101), ("identity_none", C.c_uint64),
                ("alt_hist", C.c_uint64 * 65)]

    as_dict = Report.as_dict


class PileupSums(C.Structure):
    """cl_pileup_sums: the totals of a pileup table."""
    _fields_ = [("covered", C.c_uint64), ("match", C.c_uint64), ("sub", C.c_uint64), ("del_", C.c_uint64), ("ins", C.c_uint64), ("ins_unplaced", C.c_uint64), ("reads", C.c_uint64)]
    NAMES = ("covered", "match", "sub", "del", "ins", "ins_unplaced", "reads")

    def as_dict(self):
        return {k: int(getattr(self, f[0])) for k, f in zip(self.NAMES, self._fields_)}


KSPEC_EXACT = 4096
class KSpec(C.Structure):
    """cl_kspec: the k-mer count spectrum; every field adds over disjoint key ranges except max_count (max)."""
    _fields_ = [("kmers", C.c_uint64), ("distinct", C.c_uint64), ("max_count", C.c_uint64), ("exact", C.c_uint64 * KSPEC_EXACT),
                ("big", C.c_uint64 * 33), ("big_mass", C.c_uint64 * 33)]

    as_dict = Report.as_dict


class SketchEntry(C.Structure):
    """cl_sketch_entry: one k-mer of a MinHash sketch, its cl_sketch_hash and its count."""
    _fields_ = [("hash", C.c_uint64), ("count", C.c_uint64)]


class Sketch:
    """cl_sketch: the host-side accumulator of a k-mer MinHash sketch (no device needed).  entries are strictly ascending by hash; merging is
    union by hash, counts of equal hashes add, the lowest `size` stay, `qualifying` adds."""

    def __init__(self, size: int, min_count: int):
        self.lib, self.h = load(), _P()
        st = self.lib.cl_sketch_create(size, min_count, C.byref(self.h))
        if st != CL_OK:
            raise ColordHipError(st, "cl_sketch_create failed")

    def close(self):
        if self.h:
            self.lib.cl_sketch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        size, mc, q, n = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        st = self.lib.cl_sketch_info(self.h, C.byref(size), C.byref(mc), C.byref(q), C.byref(n))
        if st != CL_OK:
            raise ColordHipError(st, "cl_sketch_info failed")
        return {"size": size.value, "min_count": mc.value, "qualifying": q.value, "n": n.value}

    def entries(self):
        """(hashes, counts) as numpy uint64 arrays"""
        import numpy as np
        n = self.info()["n"]
        buf = np.zeros((n, 2), np.uint64)
        st = self.lib.cl_sketch_entries(self.h, buf.ctypes.data if n else None, n)
        if st != CL_OK:
            raise ColordHipError(st, "cl_sketch_entries failed")
        return buf[:, 0].copy(), buf[:, 1].copy()

    def as_dict(self) -> dict:
        d = self.info()
        d["hash"], d["count"] = self.entries()
        return d

    def merge(self, hashes, counts, qualifying: int):
        """cl_sketch_merge: CL_E_INVALID (hashes not strictly ascending, a count of 0, parameters out of range) raises and merges nothing"""
        import numpy as np
        h, c = np.asarray(hashes, np.uint64), np.asarray(counts, np.uint64)
        assert h.shape == c.shape and h.ndim == 1
        buf = np.ascontiguousarray(np.stack([h, c], axis=1))
        st = self.lib.cl_sketch_merge(self.h, buf.ctypes.data if len(h) else None, len(h), qualifying)
        if st != CL_OK:
            raise ColordHipError(st, "cl_sketch_merge refused the entries")
        return self


class Overlap(C.Structure):
    """cl_overlap: one visit of a read's edit script on one reference read that holds an aligned column; twelve little-endian uint32."""
    _fields_ = [(k, C.c_uint32) for k in ("q", "t", "qlen", "tlen", "qs", "qe", "ts", "te", "matches", "subst", "anchor_bases", "flags")]


_P = C.c_void_p
class CompressParams(C.Structure):
    _fields_ = [("k", C.c_uint32), ("f", C.c_uint32), ("ci", C.c_uint32), ("cs", C.c_uint32), ("c", C.c_uint32),
                ("anchor_len", C.c_uint32), ("min_part_alt", C.c_uint32), ("max_rec", C.c_uint32), ("min_anchors", C.c_uint32),
                ("level", C.c_int32), ("source", C.c_int32), ("sparse", C.c_int32),
                ("sparse_g", C.c_double), ("sparse_exponent", C.c_double),
                ("cost_mult", C.c_double), ("frac_always", C.c_double), ("frac_min", C.c_double), ("max_matches_mult", C.c_double)]


class CompressInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_reads", "n_bases", "tot_kmers", "n_kept_kmers", "n_refs", "n_anchors", "tuple_bytes", "dna_bytes", "qual_bytes")] + \
               [("sparse_range", C.c_uint32), ("pad", C.c_uint32)]


_EXCH_GATHER_HOST = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint64))
_EXCH_A2AV = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64))
_EXCH_GATHERV = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64))


class Exchange(C.Structure):
    """cl_exchange: the collectives a multi-GPU cl_compressor calls back into (colord_amd/parallel.py fills it)."""
    _fields_ = [("user", C.c_void_p), ("rank", C.c_uint32), ("world", C.c_uint32),
                ("all_gather_host", _EXCH_GATHER_HOST), ("all_to_all_v", _EXCH_A2AV), ("all_gather_v", _EXCH_GATHERV)]


_SIG = {
    "cl_ctx_create": (C.c_int32, [C.c_int, C.POINTER(_P)]),
    "cl_ctx_destroy": (None, [_P]),
    "cl_last_error": (C.c_char_p, [_P]),
    "cl_ctx_stream": (_P, [_P]),
    "cl_ctx_last_kernel_ms": (C.c_int32, [_P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    "cl_ctx_set_timing": (None, [_P, C.c_int]),
    "cl_ctx_set_verify": (None, [_P, C.c_int]),
    "cl_ctx_verified": (C.c_int32, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cl_ctx_gap_paths": (C.c_int32, [_P, C.POINTER(C.c_uint64), C.c_uint32]),
    "cl_ctx_set_verify_streams": (None, [_P, C.c_int]),
    "cl_ctx_verified_streams": (C.c_int32, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cl_compressor_verified_streams": (C.c_int32, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cl_ctx_set_digest": (None, [_P, C.c_int]),
    "cl_ctx_digest": (C.c_int32, [_P, C.POINTER(Digest), C.POINTER(Digest)]),
    "cl_compressor_digest": (C.c_int32, [_P, C.POINTER(Digest), C.POINTER(Digest)]),
    "cl_ctx_set_digest_values": (None, [_P, C.c_int]),
    "cl_ctx_digest_values": (C.c_int32, [_P, C.POINTER(Digest)]),
    "cl_compressor_digest_values": (C.c_int32, [_P, C.POINTER(Digest)]),
    "cl_digest_qual_values": (C.c_int32, [_P, C.POINTER(QualParams), _P, _P, _P, C.c_uint64, C.POINTER(Digest)]),
    "cl_qual_values": (C.c_int32, [_P, C.POINTER(QualParams), _P, _P, _P, _P, C.c_uint64]),
    "cl_qual_values_host": (C.c_int32, [C.POINTER(QualParams), _P, _P, C.c_uint64, _P]),
    "cl_digest_qual_values_host": (C.c_int32, [_P, _P, C.c_uint64, C.c_uint64, C.POINTER(Digest)]),
    "cl_report_clear": (None, [C.POINTER(Report)]),
    "cl_report_add": (None, [C.POINTER(Report), C.POINTER(Report)]),
    "cl_report_bases": (C.c_int32, [_P, _P, C.POINTER(Report)]),
    "cl_report_quals": (C.c_int32, [_P, C.POINTER(QualParams), _P, _P, _P, C.c_uint64, C.c_uint32, C.POINTER(Report)]),
    "cl_report_bases_host": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(Report)]),
    "cl_report_quals_host": (C.c_int32, [C.POINTER(QualParams), _P, _P, C.c_uint64, C.POINTER(Report)]),
    "cl_report_values_host": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(Report)]),
    "cl_ctx_set_report": (None, [_P, C.c_int]),
    "cl_ctx_report": (C.c_int32, [_P, C.POINTER(Report)]),
    "cl_compressor_report": (C.c_int32, [_P, C.POINTER(Report)]),
    "cl_edits_clear": (None, [C.POINTER(Edits)]),
    "cl_edits_add": (None, [C.POINTER(Edits), C.POINTER(Edits)]),
    "cl_edit_profile": (C.c_int32, [_P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(Edits)]),
    "cl_edit_profile_host": (C.c_int32, [_P, _P, C.c_uint32, _P, _P, C.c_uint64, C.POINTER(Edits), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "cl_edit_profile_error": (C.c_char_p, [C.c_uint32]),
    "cl_ctx_set_edit_profile": (None, [_P, C.c_int]),
    "cl_ctx_edit_profile": (C.c_int32, [_P, C.POINTER(Edits)]),
    "cl_compressor_edit_profile": (C.c_int32, [_P, C.POINTER(Edits)]),
    "cl_kspec_clear": (None, [C.POINTER(KSpec)]),
    "cl_kspec_add": (None, [C.POINTER(KSpec), C.POINTER(KSpec)]),
    "cl_kmer_spectrum_heads": (C.c_int32, [_P, _P, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(KSpec)]),
    "cl_ctx_set_kmer_spectrum": (None, [_P, C.c_int]),
    "cl_ctx_kmer_spectrum": (C.c_int32, [_P, C.POINTER(KSpec)]),
    "cl_compressor_kmer_spectrum": (C.c_int32, [_P, C.POINTER(KSpec)]),
    "cl_sketch_hash": (C.c_uint64, [C.c_uint64]),
    "cl_sketch_create": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "cl_sketch_free": (None, [_P]),
    "cl_sketch_info": (C.c_int32, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cl_sketch_entries": (C.c_int32, [_P, _P, C.c_uint64]),
    "cl_sketch_merge": (C.c_int32, [_P, _P, C.c_uint64, C.c_uint64]),
    "cl_kmer_sketch_runs": (C.c_int32, [_P, _P, _P, C.c_uint64, C.c_uint64, C.c_uint32, _P]),
    "cl_ctx_set_kmer_sketch": (C.c_int32, [_P, C.c_int, C.c_uint32, C.c_uint32]),
    "cl_ctx_kmer_sketch": (C.c_int32, [_P, _P]),
    "cl_compressor_kmer_sketch": (C.c_int32, [_P, _P]),
    "cl_overlaps_of": (C.c_int32, [_P, _P, _P, _P, C.c_uint32, C.c_uint64, _P, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_overlaps_host": (C.c_int32, [_P, _P, C.c_uint32, _P, _P, C.c_uint64, C.c_uint64, _P, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint32)]),
    "cl_ctx_set_overlaps": (None, [_P, C.c_int]),
    "cl_ctx_overlaps": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_compressor_overlaps": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_mappings_lift": (C.c_int32, [_P, _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_mappings_lift_host": (C.c_int32, [_P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "cl_ctx_set_mappings": (None, [_P, C.c_int]),
    "cl_ctx_mappings": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_compressor_mappings": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_cigars_of": (C.c_int32, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64), _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_cigars_host": (C.c_int32, [_P, _P, C.c_uint32, _P, _P, C.c_uint64, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64), _P, C.c_uint64, C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "cl_cigars_error": (C.c_char_p, [C.c_uint32]),
    "cl_ctx_set_cigars": (C.c_int32, [_P, C.c_int]),
    "cl_ctx_cigars": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64), _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_compressor_cigars": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64), _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_cigars_pack": (C.c_int32, [_P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_cigars_pack_host": (C.c_int32, [_P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cl_cigars_unpack_host": (C.c_int32, [_P, C.c_uint64, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_cigars_check_host": (C.c_uint32, [_P, C.c_uint64]),
    "cl_cigars_refusal": (C.c_char_p, [C.c_uint32]),
    "cl_ctx_set_cigars_coded": (C.c_int32, [_P, C.c_int]),
    "cl_ctx_cigars_coded": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64), _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cl_compressor_cigars_coded": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64), _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cl_compressor_genome_geometry": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32]),
    "cl_pileup_create": (C.c_int32, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "cl_pileup_free": (None, [_P]),
    "cl_pileup_positions": (C.c_uint64, [_P]),
    "cl_pileup_add": (C.c_int32, [_P, _P, _P, _P, C.c_uint32, C.c_uint32]),
    "cl_pileup_finish": (C.c_int32, [_P]),
    "cl_pileup_columns": (C.c_int32, [_P, C.c_uint64, C.c_uint64, _P]),
    "cl_pileup_sites": (C.c_int32, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_pileup_totals": (C.c_int32, [_P, C.POINTER(PileupSums)]),
    "cl_pileup_host": (C.c_int32, [_P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, C.c_uint64,
                                   C.POINTER(C.c_uint64), C.POINTER(PileupSums), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "cl_ctx_set_pileup": (None, [_P, C.c_int]),
    "cl_compressor_pileup": (C.c_int32, [_P, C.POINTER(_P)]),
    "cl_digest_bases": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(Digest)]),
    "cl_digest_quals": (C.c_int32, [_P, C.POINTER(QualParams), _P, _P, _P, C.c_uint64, C.POINTER(Digest)]),
    "cl_digest_bases_host": (C.c_int32, [_P, _P, C.c_uint64, C.c_uint64, C.POINTER(Digest)]),
    "cl_digest_bytes_host": (C.c_int32, [C.c_uint32, _P, _P, C.c_uint64, C.c_uint64, C.POINTER(Digest)]),
    "cl_qual_decoder_set_digest": (C.c_int32, [_P, C.c_int, C.c_uint64]),
    "cl_qual_decoder_digest": (C.c_int32, [_P, C.POINTER(Digest)]),
    "cl_es_expand": (C.c_int32, [_P, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "cl_es_verify": (C.c_int32, [_P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "cl_compressor_verified": (C.c_int32, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cl_ctx_kernel_times": (C.c_int32, [_P, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_reads_pack": (C.c_int32, [_P, _P, _P, C.c_uint32, C.c_int, C.POINTER(_P)]),
    "cl_reads_free": (None, [_P]),
    "cl_reads_count": (C.c_uint32, [_P]),
    "cl_reads_total_bases": (C.c_uint64, [_P]),
    "cl_reads_total_words": (C.c_uint64, [_P]),
    "cl_reads_packed": (_P, [_P]),
    "cl_reads_invalid": (_P, [_P]),
    "cl_reads_word_offsets": (_P, [_P]),
    "cl_reads_lengths": (_P, [_P]),
    "cl_reads_has_n": (_P, [_P]),
    "cl_reads_compact": (C.c_int32, [_P, _P, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_kmer_scan": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_kmer_count_filter": (C.c_int32, [_P, _P, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P), C.POINTER(KmerStats)]),
    "cl_kmer_set_create": (C.c_int32, [_P, _P, _P, C.c_uint64, C.c_uint32, C.POINTER(_P)]),
    "cl_kmer_set_free": (None, [_P]),
    "cl_kmer_set_size": (C.c_uint64, [_P]),
    "cl_kmer_set_keys": (_P, [_P]),
    "cl_kmer_set_counts": (_P, [_P]),
    "cl_kmer_set_check": (C.c_int32, [_P, _P, _P, C.c_uint64, _P]),
    "cl_accepted_kmers": (C.c_int32, [_P, _P, _P, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "cl_kmer_lists_free": (None, [_P]),
    "cl_kmer_lists_reads": (C.c_uint32, [_P]),
    "cl_kmer_lists_total": (C.c_uint64, [_P]),
    "cl_kmer_lists_offsets": (_P, [_P]),
    "cl_kmer_lists_kmers": (_P, [_P]),
    "cl_kmer_lists_ids": (_P, [_P]),
    "cl_kmer_lists_pos": (_P, [_P]),
    "cl_ref_accept": (C.c_int32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, _P]),
    "cl_index_build": (C.c_int32, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "cl_index_entries_of": (C.c_int32, [_P, _P, _P, C.c_uint32, _P, _P, C.c_uint64, C.POINTER(C.c_uint64), _P, C.POINTER(C.c_uint32)]),
    "cl_index_build_pairs": (C.c_int32, [_P, _P, _P, _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "cl_index_free": (None, [_P]),
    "cl_index_n_refs": (C.c_uint32, [_P]),
    "cl_index_entries": (C.c_uint64, [_P]),
    "cl_index_ref_rank": (_P, [_P]),
    "cl_candidates": (C.c_int32, [_P, _P, _P, C.c_uint32, _P, _P, _P]),
    "cl_candidates_common": (C.c_int32, [_P, _P, _P, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_qual_coder_create": (C.c_int32, [_P, C.POINTER(QualParams), C.POINTER(_P)]),
    "cl_qual_coder_ctx": (_P, [_P]),
    "cl_qual_coder_free": (None, [_P]),
    "cl_qual_coder_set_domain_symbols": (C.c_int32, [_P, C.c_uint64]),
    "cl_qual_coder_domains": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_qual_coder_model": (C.c_int32, [_P, C.c_uint32, C.c_uint64, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    "cl_qual_coder_groups": (C.c_int32, [_P, C.POINTER(C.c_uint64)]),
    "cl_compressor_set_qual_domain_symbols": (C.c_int32, [_P, C.c_uint64]),
    "cl_compressor_qual_domains": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_qual_decode_domains": (C.c_int32, [_P, C.POINTER(QualParams), _P, _P, _P, C.c_uint64, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, _P, C.c_uint64, _P, C.c_uint64]),
    "cl_qual_encode": (C.c_int32, [_P, _P, _P, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "cl_anchor_candidates": (C.c_int32, [_P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_uint32, C.POINTER(_P)]),
    "cl_anchor_candidates_hifi": (C.c_int32, [_P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, C.POINTER(_P)]),
    "cl_anchors_free": (None, [_P]),
    "cl_anchors_total": (C.c_uint64, [_P]),
    "cl_anchors_wave_tasks": (C.c_uint64, [_P]),
    "cl_anchors_wave_pairs": (C.c_uint64, [_P]),
    "cl_anchors_lane_tasks": (C.c_uint64, [_P]),
    "cl_anchors_lane_pairs": (C.c_uint64, [_P]),
    "cl_anchors_n_cands": (_P, [_P]),
    "cl_anchors_cands": (_P, [_P]),
    "cl_anchors_cand_offsets": (_P, [_P]),
    "cl_anchors_data": (_P, [_P]),
    "cl_encode_plain": (C.c_int32, [_P, _P, _P, C.c_uint64, _P, _P, C.POINTER(C.c_uint64)]),
    "cl_reads_select": (C.c_int32, [_P, _P, _P, C.POINTER(_P)]),
    "cl_reads_from_arena": (C.c_int32, [_P, _P, _P, _P, C.c_uint32, C.POINTER(_P)]),
    "cl_estimator_logs": (C.c_int32, [_P, _P, _P, C.c_uint64, _P]),
    "cl_es_flags": (C.c_int32, [_P, _P, _P, _P, _P, _P]),
    "cl_id_coder_create": (C.c_int32, [C.c_int32, C.POINTER(_P)]),
    "cl_id_coder_free": (None, [_P]),
    "cl_id_coder_error": (C.c_char_p, [_P]),
    "cl_id_encode_part": (C.c_int32, [_P, _P, _P, _P, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_compress_shard": (C.c_int32, [_P, C.POINTER(CompressParams), _P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, _P, _P, C.c_uint64, _P, _P, C.c_uint64, _P,
                                      C.POINTER(CompressInfo)]),
    "cl_candidates_at": (C.c_int32, [_P, _P, _P, _P, C.c_uint32, _P, _P, _P]),
    "cl_compressor_create": (C.c_int32, [_P, _P, C.POINTER(CompressParams), C.POINTER(QualParams), C.POINTER(Exchange), C.c_uint64, C.POINTER(_P)]),
    "cl_compressor_free": (None, [_P]),
    "cl_compressor_count_add": (C.c_int32, [_P, _P]),
    "cl_compressor_count_finish": (C.c_int32, [_P, C.POINTER(KmerStats)]),
    "cl_compressor_refs_add": (C.c_int32, [_P, _P]),
    "cl_compressor_refs_finish": (C.c_int32, [_P]),
    "cl_compressor_encode": (C.c_int32, [_P, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint64, _P, _P, C.c_uint64, _P, C.POINTER(CompressInfo)]),
    "cl_compressor_genome_add": (C.c_int32, [_P, _P]),
    "cl_compressor_pseudo_reads": (C.c_int32, [_P, _P]),
    "cl_genome_encode": (C.c_int32, [_P, _P, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_genome_decode": (C.c_int32, [_P, C.c_uint64, C.c_uint32, _P, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "cl_genome_md5": (C.c_int32, [_P, _P, C.c_uint32, _P]),
    "cl_compressor_prepare": (C.c_int32, [_P, _P, _P, C.c_uint32]),
    "cl_compressor_prepare_parts": (C.c_int32, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, _P]),
    "cl_compressor_info": (C.c_int32, [_P, C.POINTER(KmerStats), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "cl_dna_decoder_create": (C.c_int32, [C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.c_double, C.POINTER(_P)]),
    "cl_dna_decoder_free": (None, [_P]),
    "cl_dna_decoder_error": (C.c_char_p, [_P]),
    "cl_dna_decoder_add_ref": (C.c_int32, [_P, _P, C.c_uint32]),
    "cl_dna_decoder_new_domain": (C.c_int32, [_P]),
    "cl_dna_decode_part": (C.c_int32, [_P, _P, C.c_uint64, C.c_uint32, _P, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "cl_qual_decoder_create": (C.c_int32, [C.POINTER(QualParams), C.POINTER(_P)]),
    "cl_qual_decoder_free": (None, [_P]),
    "cl_qual_decoder_new_domain": (C.c_int32, [_P]),
    "cl_qual_decode_part": (C.c_int32, [_P, _P, C.c_uint64, _P, _P, C.c_uint32, _P]),
    "cl_id_decoder_create": (C.c_int32, [C.c_int32, C.POINTER(_P)]),
    "cl_id_decoder_free": (None, [_P]),
    "cl_id_decode_part": (C.c_int32, [_P, _P, C.c_uint64, C.c_uint32, _P, C.c_uint64, _P, _P, C.POINTER(C.c_uint64)]),
    "cl_encode_reads": (C.c_int32, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, _P, C.c_uint32, _P, C.c_uint64, _P, _P, C.POINTER(C.c_uint64)]),
    "cl_dna_coder_create": (C.c_int32, [_P, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(_P)]),
    "cl_dna_coder_free": (None, [_P]),
    "cl_dna_coder_model": (C.c_int32, [_P, C.c_uint32, C.c_uint64, _P]),
    "cl_dna_encode": (C.c_int32, [_P, _P, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "cl_sort_u64": (C.c_int32, [_P, _P, C.c_uint64, C.c_uint32, C.c_uint32]),
    "cl_sort_u64_u32": (C.c_int32, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32]),
    "cl_sort_u32": (C.c_int32, [_P, _P, C.c_uint64, C.c_uint32, C.c_uint32]),
    "cl_sort_u32_u32": (C.c_int32, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32]),
    "cl_sort_swap_u32_u32": (C.c_int32, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P]),
    "cl_sort_swap_u64_u32": (C.c_int32, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P]),
    "cl_scan_u32": (C.c_int32, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_scan_u32_u64": (C.c_int32, [_P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_run_starts_u32": (C.c_int32, [_P, _P, C.c_uint64, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cl_run_starts_u64": (C.c_int32, [_P, _P, C.c_uint64, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
}

_lib = None


def load():
    """Load libcolord_hip.so and declare every entry point of include/colord_hip.h.  Fails loudly."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ColordHipError(CL_E_HIP, f"{LIB_PATH} is missing: run `make -C colord_amd/csrc` "
                                 "(or __graft_entry__.build()); there is no CPU fallback")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIG.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def exported_names():
    return sorted(_SIG)
