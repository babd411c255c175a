"""Thin object layer over the C ABI for tests and bench.py: torch tensors own the caller-side device
memory; everything computed comes from the HIP library (no CPU fallback anywhere)."""
from __future__ import annotations
import ctypes as C
import numpy as np
import torch
from . import _native as N


def _check(ctx, st):
    if ctx is not None and getattr(ctx, "timing", False):
        for n, (ms, k, b, cells) in ctx.kernel_times().items():
            a = ctx.acc.setdefault(n, [0.0, 0, 0.0, 0.0])
            a[0] += ms
            a[1] += k
            a[2] += b
            a[3] += cells
    if st != N.CL_OK:
        msg = N.load().cl_last_error(ctx.h).decode() if ctx is not None and ctx.h else ""
        raise N.ColordHipError(st, msg)


def _view(ptr, n, dtype, device):
    """Copy n elements of a library-owned device array into a new torch tensor."""
    out = torch.empty(int(n), dtype=dtype, device=device)
    if n:
        torch.cuda.synchronize(device)
        rc = _hip().hipMemcpy(C.c_void_p(out.data_ptr()), C.c_void_p(ptr), C.c_size_t(int(n) * out.element_size()), 3)  # D2D
        if rc != 0:
            raise N.ColordHipError(N.CL_E_HIP, f"hipMemcpy failed ({rc})")
    return out


_HIP = None


def _hip():
    global _HIP
    if _HIP is None:
        _HIP = C.CDLL("libamdhip64.so")
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _HIP.hipMemcpy.restype = C.c_int
    return _HIP


class _OrderedLib:
    """The C ABI as this binding calls it: every entry point first waits for torch's current stream on the device.  The library works
    on streams of its own (non-blocking: nothing orders them after torch's), so a tensor torch is still computing — offsets rebased by a
    subtraction, a slice made contiguous — could be read by the library before it was written.  That was the one unexplained failure of
    round 4 (`cl_reads_pack: offsets not monotone` once in seven runs of test_chunked_equals_one_call_200_mbases; reproduced at will under
    COLORD_HIP_SYNC_DEBUG, which shifts the timing): a race of the HARNESS, not of the library's pool.  Waiting on an idle stream costs
    microseconds; a host that embeds the library orders its own streams."""
    _HOST_ONLY = ("cl_last_error", "cl_ctx_kernel_times", "cl_ctx_last_kernel_ms", "cl_ctx_set_timing", "cl_ref_accept", "cl_ctx_set_verify", "cl_ctx_verified",
                  "cl_compressor_verified", "cl_ctx_set_verify_streams", "cl_ctx_verified_streams", "cl_compressor_verified_streams",
                  "cl_ctx_set_digest", "cl_ctx_digest", "cl_compressor_digest", "cl_digest_bases_host", "cl_digest_bytes_host", "cl_qual_decoder_set_digest", "cl_qual_decoder_digest",
                  "cl_ctx_set_digest_values", "cl_ctx_digest_values", "cl_compressor_digest_values", "cl_qual_values_host", "cl_digest_qual_values_host",
                  "cl_qual_coder_domains", "cl_compressor_qual_domains", "cl_ctx_gap_paths",
                  "cl_report_clear", "cl_report_add", "cl_report_bases_host", "cl_report_quals_host", "cl_report_values_host", "cl_ctx_set_report", "cl_ctx_report", "cl_compressor_report",
                  "cl_edits_clear", "cl_edits_add", "cl_edit_profile_host", "cl_edit_profile_error", "cl_ctx_set_edit_profile", "cl_ctx_edit_profile", "cl_compressor_edit_profile",
                  "cl_kspec_clear", "cl_kspec_add", "cl_ctx_set_kmer_spectrum", "cl_ctx_kmer_spectrum", "cl_compressor_kmer_spectrum",
                  "cl_sketch_hash", "cl_sketch_create", "cl_sketch_info", "cl_sketch_entries", "cl_sketch_merge", "cl_ctx_set_kmer_sketch", "cl_ctx_kmer_sketch", "cl_compressor_kmer_sketch",
                  "cl_overlaps_host", "cl_ctx_set_overlaps", "cl_ctx_overlaps", "cl_compressor_overlaps",
                  "cl_mappings_lift_host", "cl_ctx_set_mappings", "cl_ctx_mappings", "cl_compressor_mappings",
                  "cl_cigars_host", "cl_cigars_error", "cl_ctx_set_cigars", "cl_ctx_cigars", "cl_compressor_cigars",
                  "cl_cigars_pack_host", "cl_cigars_unpack_host", "cl_cigars_check_host", "cl_cigars_refusal", "cl_ctx_set_cigars_coded", "cl_ctx_cigars_coded", "cl_compressor_cigars_coded",
                  "cl_pileup_host", "cl_pileup_positions", "cl_ctx_set_pileup")

    def __init__(self, lib, device):
        self._lib, self._device, self._cache = lib, device, {}

    def __getattr__(self, name):
        f = self._cache.get(name)
        if f is None:
            raw = getattr(self._lib, name)
            if not name.startswith("cl_") or name in self._HOST_ONLY or name.endswith("_free") or name.endswith("_destroy"):
                f = raw
            else:
                dev = self._device

                def f(*a, _raw=raw, _dev=dev):
                    torch.cuda.current_stream(_dev).synchronize()
                    return _raw(*a)
            self._cache[name] = f
        return f


class Context:
    def __init__(self, device: int = 0, timing: bool = False):
        self.lib = N.load()
        if not torch.cuda.is_available():
            raise N.ColordHipError(N.CL_E_HIP, "no GPU visible: the HIP path cannot run (no CPU fallback)")
        self.h = N._P()
        st = self.lib.cl_ctx_create(device, C.byref(self.h))
        if st != N.CL_OK:
            raise N.ColordHipError(st, "cl_ctx_create failed")
        self.device = torch.device("cuda", device)
        self.lib = _OrderedLib(self.lib, self.device)
        self.timing = timing
        self.acc = {}                  # {kernel: [ms, launches]} accumulated over API calls while timing is on
        if timing:
            self.lib.cl_ctx_set_timing(self.h, 1)

    def close(self):
        if self.h:
            self.lib.cl_ctx_destroy(self.h)
            self.h = None

    def kernel_ms(self, name: str):
        ms, n = C.c_double(0), C.c_uint32(0)
        self.lib.cl_ctx_last_kernel_ms(self.h, name.encode(), C.byref(ms), C.byref(n))
        return ms.value, n.value

    def kernel_times(self) -> dict:
        """{kernel: (ms, launches)} of the last API call (timing must be on)."""
        buf = C.create_string_buffer(1 << 16)
        need = C.c_uint64(0)
        if self.lib.cl_ctx_kernel_times(self.h, buf, len(buf), C.byref(need)) != N.CL_OK:
            return {}
        out = {}
        for line in buf.value.decode().splitlines():
            f = line.split("\t")
            out[f[0]] = (float(f[1]), int(f[2]), float(f[3]), float(f[4]) if len(f) > 4 else 0.0)
        return out

    def set_verify(self, on: bool = True):
        """cl_ctx_set_verify: compress_shard() and compressors of this context rebuild every read from its edit script and compare it
        with the input (ColordHipError with status CL_E_MISMATCH names the first read that differs)."""
        self.lib.cl_ctx_set_verify(self.h, int(bool(on)))

    def verified(self):
        """(reads, bases) checked so far on this context and the encode lanes of its compressor."""
        r, b = C.c_uint64(0), C.c_uint64(0)
        _check(None, self.lib.cl_ctx_verified(self.h, C.byref(r), C.byref(b)))
        return r.value, b.value

    def gap_paths(self):
        """cl_ctx_gap_paths of the last encode_reads(): {"classes": gaps per size class 0..7, "quad_to_wave", "giant_to_wave",
        "wave_redo_rounds"} summed over the recursion levels."""
        out = (C.c_uint64 * 11)()
        _check(None, self.lib.cl_ctx_gap_paths(self.h, out, 11))
        v = [int(x) for x in out]
        return {"classes": v[:8], "quad_to_wave": v[8], "giant_to_wave": v[9], "wave_redo_rounds": v[10]}

    def set_verify_streams(self, on: bool = True):
        """cl_ctx_set_verify_streams: the DNA and quality coders of this context decode every coded part on the device against the
        intervals its models gave (ColordHipError with status CL_E_MISMATCH names the stream, the part and the symbol).  The models
        themselves are not replayed."""
        self.lib.cl_ctx_set_verify_streams(self.h, int(bool(on)))

    def verified_streams(self):
        """(parts, symbols, bytes) of the coded streams checked so far by the coders on this context."""
        p, s, b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(None, self.lib.cl_ctx_verified_streams(self.h, C.byref(p), C.byref(s), C.byref(b)))
        return p.value, s.value, b.value

    def set_digest(self, on: bool = True):
        """cl_ctx_set_digest: compress_shard() and compressors of this context digest the bases and quality symbols of their input."""
        self.lib.cl_ctx_set_digest(self.h, int(bool(on)))

    def digest(self):
        """cl_ctx_digest: ((reads, symbols, sum) of the dna digest, the same of the qual digest) so far on this context."""
        d, q = N.Digest(), N.Digest()
        _check(None, self.lib.cl_ctx_digest(self.h, C.byref(d), C.byref(q)))
        return d.triple(), q.triple()

    def digest_bases(self, reads: "Reads", first_read: int = 0, acc: "N.Digest | None" = None):
        """cl_digest_bases: the dna digest of an arena whose first read is read first_read of the input, added to acc; (reads, symbols, sum)."""
        acc = N.Digest() if acc is None else acc
        _check(self, self.lib.cl_digest_bases(self.h, reads.h, first_read, C.byref(acc)))
        return acc.triple()

    def digest_quals(self, reads: "Reads", quals: torch.Tensor, qual_off: torch.Tensor, mode: int, fwd=(), first_read: int = 0, acc: "N.Digest | None" = None):
        """cl_digest_quals: the qual digest of the symbols a quality coder of `mode` (thresholds fwd) codes for the reads, added to acc."""
        prm = N.QualParams()
        prm.mode, prm.source, prm.level, prm.n_fwd = mode, 0, 1, len(fwd)
        for i, v in enumerate(fwd):
            prm.fwd[i] = v
        acc = N.Digest() if acc is None else acc
        quals, qual_off = quals.contiguous(), qual_off.contiguous()
        _check(self, self.lib.cl_digest_quals(self.h, C.byref(prm), reads.h, quals.data_ptr() if quals.numel() else None, qual_off.data_ptr(), first_read, C.byref(acc)))
        return acc.triple()

    def set_digest_values(self, on: bool = True):
        """cl_ctx_set_digest_values: compress_shard() and compressors of this context digest the quality VALUES their input will decode to."""
        self.lib.cl_ctx_set_digest_values(self.h, int(bool(on)))

    def digest_values(self):
        """cl_ctx_digest_values: (reads, symbols, sum) of the qual-values digest so far on this context."""
        d = N.Digest()
        _check(None, self.lib.cl_ctx_digest_values(self.h, C.byref(d)))
        return d.triple()

    def set_report(self, on: bool = True):
        """cl_ctx_set_report: compress_shard() and compressors of this context add the content report of their input (cleared when switched on)."""
        self.lib.cl_ctx_set_report(self.h, int(bool(on)))

    def report(self) -> "N.Report":
        """cl_ctx_report: the report so far on this context."""
        r = N.Report()
        _check(None, self.lib.cl_ctx_report(self.h, C.byref(r)))
        return r

    def set_edit_profile(self, on: bool = True):
        """cl_ctx_set_edit_profile: every batch of tuple streams made on this context or by a lane of its compressors adds its edit-operation profile
        (cleared when switched on)."""
        self.lib.cl_ctx_set_edit_profile(self.h, int(bool(on)))

    def edit_profile(self) -> "N.Edits":
        """cl_ctx_edit_profile: the profile so far of this context and its compressor's encode lanes."""
        e = N.Edits()
        _check(None, self.lib.cl_ctx_edit_profile(self.h, C.byref(e)))
        return e

    def edit_profile_of(self, refs: "Reads", es: torch.Tensor, es_off: torch.Tensor, flush_bytes: int = 0, max_blocks: int = 0, acc: "N.Edits | None" = None) -> "N.Edits":
        """cl_edit_profile: the profile of the tuple streams es / es_off (n + 1 byte offsets) against the arena refs, added to acc.  A malformed
        stream raises (CL_E_INVALID, the text names the first such read) and leaves acc as it is."""
        es, es_off = es.contiguous(), es_off.contiguous()
        if acc is None:
            acc = N.Edits()
            self.lib.cl_edits_clear(C.byref(acc))
        n = max(es_off.numel() - 1, 0)
        _check(self, self.lib.cl_edit_profile(self.h, refs.h, es.data_ptr() if es.numel() else None, es_off.data_ptr() if n else None, n, flush_bytes, max_blocks, C.byref(acc)))
        return acc

    def set_overlaps(self, on: bool = True):
        """cl_ctx_set_overlaps: every batch of tuple streams made on this context or by a lane of its compressors leaves its overlap records
        (dropped when switched on)."""
        self.lib.cl_ctx_set_overlaps(self.h, int(bool(on)))

    def overlaps(self) -> np.ndarray:
        """cl_ctx_overlaps: the records so far of this context and its compressor's encode lanes in input order, (n, 12) uint32 in the field
        order of cl_overlap."""
        return _overlap_records(self.lib.cl_ctx_overlaps, self.h)

    def overlaps_of(self, refs: "Reads", es: torch.Tensor, es_off: torch.Tensor, first_read: int = 0, ref_read: "torch.Tensor | None" = None, max_blocks: int = 0,
                    cap: "int | None" = None) -> torch.Tensor:
        """cl_overlaps_of: the overlap records of the tuple streams es / es_off (n + 1 byte offsets) against the arena refs, (n, 12) int32 on the
        device (the bits of uint32, field order of cl_overlap).  ref_read: reference id -> input index (a 4-byte dtype on the device).  With cap
        the call is made once with room for cap records (CL_E_CAPACITY raises); without, the need is asked for first.  A malformed stream
        raises (CL_E_INVALID, the text names the first such read)."""
        es, es_off = es.contiguous(), es_off.contiguous()
        n = max(es_off.numel() - 1, 0)
        if ref_read is not None:
            assert ref_read.element_size() == 4
            ref_read = ref_read.contiguous()
        args = (self.h, refs.h, es.data_ptr() if es.numel() else None, es_off.data_ptr() if n else None, n, first_read,
                ref_read.data_ptr() if ref_read is not None and ref_read.numel() else None, ref_read.numel() if ref_read is not None else 0, max_blocks)
        need = C.c_uint64(0)
        if cap is None:
            st = self.lib.cl_overlaps_of(*args, None, 0, C.byref(need))
            if st not in (N.CL_OK, N.CL_E_CAPACITY):
                _check(self, st)
            cap = need.value
        out = torch.empty((cap, 12), dtype=torch.int32, device=self.device)
        _check(self, self.lib.cl_overlaps_of(*args, out.data_ptr() if cap else None, cap, C.byref(need)))
        return out[:need.value]

    def cigars_of(self, refs: "Reads", es: torch.Tensor, es_off: torch.Tensor, id_limit: int = 0, max_blocks: int = 0, caps: "tuple | None" = None):
        """cl_cigars_of: the CIGARs of the records of cl_overlaps_of over the same streams: (the operation count per record, the operations
        len << 4 | op of the records one behind the other), two int32 tensors on the device (the bits of uint32).  id_limit: a record on a
        reference id at or past it gets the count 0 (0: every reference).  With caps = (records, operations) the call is made once with that
        room (CL_E_CAPACITY raises); without, the needs are asked for first.  A malformed stream raises as in overlaps_of."""
        es, es_off = es.contiguous(), es_off.contiguous()
        n = max(es_off.numel() - 1, 0)
        args = (self.h, refs.h, es.data_ptr() if es.numel() else None, es_off.data_ptr() if n else None, n, id_limit, max_blocks)
        nr, no = C.c_uint64(0), C.c_uint64(0)
        if caps is None:
            st = self.lib.cl_cigars_of(*args, None, 0, C.byref(nr), None, 0, C.byref(no))
            if st not in (N.CL_OK, N.CL_E_CAPACITY):
                _check(self, st)
            caps = (nr.value, no.value)
        rec = torch.empty(caps[0], dtype=torch.int32, device=self.device)
        ops = torch.empty(caps[1], dtype=torch.int32, device=self.device)
        _check(self, self.lib.cl_cigars_of(*args, rec.data_ptr() if caps[0] else None, caps[0], C.byref(nr), ops.data_ptr() if caps[1] else None, caps[1], C.byref(no)))
        return rec[:nr.value], ops[:no.value]

    def set_cigars(self, on: bool = True):
        """cl_ctx_set_cigars: on top of set_mappings, every batch leaves the CIGARs of its lifted records too (dropped when switched on);
        refused without set_mappings."""
        _check(self, self.lib.cl_ctx_set_cigars(self.h, int(bool(on))))

    def cigars(self):
        """cl_ctx_cigars: (a count per record of mappings(), the operations one behind the other), two uint32 arrays."""
        return _cigar_records(self.lib.cl_ctx_cigars, self.h)

    def cigars_pack(self, ops: torch.Tensor, part_ops: int = 0, seg_ops: int = 0, cap: "int | None" = None) -> bytes:
        """cl_cigars_pack: the operation words in `ops` (an int32 tensor on the device, the bits of uint32) as the bytes of their coded segments
        (DESIGN.md 4p); a knob of 0 is its default.  With `cap` the call is made once with that room (CL_E_CAPACITY raises); without, the need
        is asked for first.  A word that is no operation raises CL_E_INVALID, the text naming its index."""
        ops = ops.contiguous()
        n, nb = ops.numel(), C.c_uint64(0)
        args = (self.h, ops.data_ptr() if n else None, n, part_ops, seg_ops)
        if cap is None:
            st = self.lib.cl_cigars_pack(*args, None, 0, C.byref(nb))
            if st not in (N.CL_OK, N.CL_E_CAPACITY):
                _check(self, st)
            cap = nb.value
        out = np.zeros(max(cap, 1), np.uint8)
        _check(self, self.lib.cl_cigars_pack(*args, out.ctypes.data, cap, C.byref(nb)))
        return out[:nb.value].tobytes()

    def set_cigars_coded(self, on: bool = True):
        """cl_ctx_set_cigars_coded: on top of set_cigars, a batch's operations are coded on the device and kept as segment bytes; refused
        without set_cigars."""
        _check(self, self.lib.cl_ctx_set_cigars_coded(self.h, int(bool(on))))

    def cigars_coded(self):
        """cl_ctx_cigars_coded: (a count per record of mappings(), the coded segments of all batches, their operations, their segments)."""
        return _cigar_coded(self.lib.cl_ctx_cigars_coded, self.h)

    def set_mappings(self, on: bool = True):
        """cl_ctx_set_mappings: every batch of tuple streams made by a compressor of this context (one with pseudo reads and their geometry)
        leaves its records on genome pieces, lifted to the genome's sequences (dropped when switched on)."""
        self.lib.cl_ctx_set_mappings(self.h, int(bool(on)))

    def mappings(self) -> np.ndarray:
        """cl_ctx_mappings: the lifted records so far of this context and its compressor's encode lanes in input order, (n, 12) uint32 in the
        field order of cl_overlap."""
        return _overlap_records(self.lib.cl_ctx_mappings, self.h)

    def mappings_lift(self, recs: torch.Tensor, seq_len, read_len: int, overlap: int, cap: "int | None" = None) -> torch.Tensor:
        """cl_mappings_lift: the (n, 12) int32 records on the device whose target is a genome piece, lifted to the sequences of seq_len (host),
        (m, 12) int32 on the device.  With cap the call is made once with room for cap records (CL_E_CAPACITY raises); without, the need is
        asked for first.  A refused record raises (CL_E_INVALID, the text names the first)."""
        recs = recs.contiguous()
        n = recs.numel() // 12
        sl = np.ascontiguousarray(np.asarray(seq_len, dtype=np.uint64))
        args = (self.h, recs.data_ptr() if n else None, n, sl.ctypes.data if len(sl) else None, len(sl), read_len, overlap)
        need = C.c_uint64(0)
        if cap is None:
            st = self.lib.cl_mappings_lift(*args, None, 0, C.byref(need))
            if st not in (N.CL_OK, N.CL_E_CAPACITY):
                _check(self, st)
            cap = need.value
        out = torch.empty((cap, 12), dtype=torch.int32, device=self.device)
        _check(self, self.lib.cl_mappings_lift(*args, out.data_ptr() if cap else None, cap, C.byref(need)))
        return out[:need.value]

    def set_pileup(self, on: bool = True):
        """cl_ctx_set_pileup: a compressor of this context (one with pseudo reads and their geometry) makes one table of per-position base counts
        in refs_finish(), and every batch of tuple streams it makes is added to it (Compressor.pileup)."""
        self.lib.cl_ctx_set_pileup(self.h, int(bool(on)))

    def pileup(self, refs: "Reads", seq_len, read_len: int, overlap: int) -> "Pileup":
        """cl_pileup_create: the zeroed table for the genome whose pieces are the first reads of the arena refs, which must outlive finish()."""
        sl = np.ascontiguousarray(np.asarray(seq_len, dtype=np.uint64))
        h = N._P()
        _check(self, self.lib.cl_pileup_create(self.h, refs.h, sl.ctypes.data if len(sl) else None, len(sl), read_len, overlap, C.byref(h)))
        return Pileup(self, h)

    def set_kmer_spectrum(self, on: bool = True):
        """cl_ctx_set_kmer_spectrum: every count_filter() on this context, and the pass 1 of its compressors, adds the count spectrum of the
        k-mers it counted, before the cut at ci and the saturation at cs (cleared when switched on)."""
        self.lib.cl_ctx_set_kmer_spectrum(self.h, int(bool(on)))

    def kmer_spectrum(self) -> dict:
        """cl_ctx_kmer_spectrum: the spectrum so far on this context, as ints and numpy uint64 arrays (N.KSpec's fields)."""
        s = N.KSpec()
        _check(None, self.lib.cl_ctx_kmer_spectrum(self.h, C.byref(s)))
        return s.as_dict()

    def kmer_spectrum_heads(self, head_pos: torch.Tensor, n: int, max_blocks: int = 0, acc: "N.KSpec | None" = None) -> "N.KSpec":
        """cl_kmer_spectrum_heads: the spectrum of the runs that start at the ascending positions head_pos (uint32 values, in a 4-byte dtype) of
        a sorted array of n keys, added to acc.  Malformed positions raise (CL_E_INVALID) and leave acc as it is."""
        assert head_pos.element_size() == 4
        head_pos = head_pos.contiguous()
        if acc is None:
            acc = N.KSpec()
            self.lib.cl_kspec_clear(C.byref(acc))
        _check(self, self.lib.cl_kmer_spectrum_heads(self.h, head_pos.data_ptr() if head_pos.numel() else None, head_pos.numel(), n, max_blocks, C.byref(acc)))
        return acc

    def set_kmer_sketch(self, on: bool = True, size: int = 10000, min_count: int = 2):
        """cl_ctx_set_kmer_sketch: every count_filter() on this context, and the pass 1 of its compressors, merges the MinHash sketch of the
        k-mers it counted at least min_count times (emptied, and its parameters set, when switched on)."""
        _check(self, self.lib.cl_ctx_set_kmer_sketch(self.h, int(bool(on)), size, min_count))

    def kmer_sketch(self) -> dict:
        """cl_ctx_kmer_sketch: the sketch so far on this context: size, min_count, qualifying, n and the entries as numpy uint64 arrays."""
        s = N.Sketch(0, 0)
        _check(None, self.lib.cl_ctx_kmer_sketch(self.h, s.h))
        return s.as_dict()

    def kmer_sketch_runs(self, keys: torch.Tensor, head_pos: torch.Tensor, n: int, acc: "N.Sketch", max_blocks: int = 0) -> "N.Sketch":
        """cl_kmer_sketch_runs: the sketch of the runs that start at the ascending positions head_pos (uint32 values, in a 4-byte dtype) of the
        sorted array keys (64-bit) of n keys, merged into acc with acc's size and min_count.  A refusal raises (CL_E_INVALID) and leaves acc
        as it is."""
        assert head_pos.element_size() == 4 and keys.element_size() == 8
        keys, head_pos = keys.contiguous(), head_pos.contiguous()
        _check(self, self.lib.cl_kmer_sketch_runs(self.h, keys.data_ptr() if keys.numel() else None, head_pos.data_ptr() if head_pos.numel() else None,
                                                  head_pos.numel(), n, max_blocks, acc.h))
        return acc

    @staticmethod
    def new_report() -> "N.Report":
        r = N.Report()
        N.load().cl_report_clear(C.byref(r))
        return r

    def report_bases(self, reads: "Reads", acc: "N.Report | None" = None) -> "N.Report":
        """cl_report_bases: reads, bases, base composition and read lengths of an arena, added to acc."""
        acc = self.new_report() if acc is None else acc
        _check(self, self.lib.cl_report_bases(self.h, reads.h, C.byref(acc)))
        return acc

    def report_quals(self, reads: "Reads", quals: torch.Tensor, qual_off: torch.Tensor, mode: int, fwd=(), rev=(), flush_bytes: int = 0, max_blocks: int = 0,
                     acc: "N.Report | None" = None) -> "N.Report":
        """cl_report_quals: input quality against the value a decoder of `mode` (thresholds fwd, -D values rev) will write, and the reads' mean
        qualities, added to acc.  flush_bytes / max_blocks (0: the defaults) change no result."""
        prm = self._qual_params(mode, fwd, rev)
        acc = self.new_report() if acc is None else acc
        quals, qual_off = quals.contiguous(), qual_off.contiguous()
        _check(self, self.lib.cl_report_quals(self.h, C.byref(prm), reads.h, quals.data_ptr() if quals.numel() else None, qual_off.data_ptr(), flush_bytes, max_blocks, C.byref(acc)))
        return acc

    @staticmethod
    def _qual_params(mode, fwd, rev):
        prm = N.QualParams()
        prm.mode, prm.source, prm.level, prm.n_fwd, prm.n_rev = mode, 0, 1, len(fwd), len(rev)
        for i, v in enumerate(fwd):
            prm.fwd[i] = v
        for i, v in enumerate(rev):
            prm.rev[i] = v
        return prm

    def digest_qual_values(self, reads: "Reads", quals: torch.Tensor, qual_off: torch.Tensor, mode: int, fwd=(), rev=(), first_read: int = 0, acc: "N.Digest | None" = None):
        """cl_digest_qual_values: the qual-values digest of what a decoder of `mode` (thresholds fwd, -D values rev) will write for the reads, added to acc."""
        prm = self._qual_params(mode, fwd, rev)
        acc = N.Digest() if acc is None else acc
        quals, qual_off = quals.contiguous(), qual_off.contiguous()
        _check(self, self.lib.cl_digest_qual_values(self.h, C.byref(prm), reads.h, quals.data_ptr() if quals.numel() else None, qual_off.data_ptr(), first_read, C.byref(acc)))
        return acc.triple()

    def qual_values(self, reads: "Reads", quals: torch.Tensor, qual_off: torch.Tensor, mode: int, fwd=(), rev=(), out: "torch.Tensor | None" = None):
        """cl_qual_values: the ASCII quality bytes a decoder of `mode` will write for the reads, at the offsets of qual_off; `out` (a uint8
        tensor on the device, made here when None) may be larger than the last offset — one that is smaller raises CL_E_CAPACITY."""
        prm = self._qual_params(mode, fwd, rev)
        quals, qual_off = quals.contiguous(), qual_off.contiguous()
        if out is None:
            out = torch.empty(int(qual_off[-1]) if qual_off.numel() else 0, dtype=torch.uint8, device=quals.device)
        _check(self, self.lib.cl_qual_values(self.h, C.byref(prm), reads.h, quals.data_ptr() if quals.numel() else None, qual_off.data_ptr(),
                                             out.data_ptr() if out.numel() else None, out.numel()))
        return out

    # ---- arena ----
    def pack_reads(self, codes: torch.Tensor, offsets: torch.Tensor, ascii: bool = False) -> "Reads":
        assert codes.dtype == torch.uint8 and offsets.dtype in (torch.int64, torch.uint64)
        codes = codes.to(self.device).contiguous()
        offsets = offsets.to(self.device).contiguous()
        h = N._P()
        _check(self, self.lib.cl_reads_pack(self.h, codes.data_ptr(), offsets.data_ptr(), offsets.numel() - 1, int(ascii), C.byref(h)))
        return Reads(self, h)

    def select_reads(self, reads: "Reads", keep: torch.Tensor) -> "Reads":
        """CReferenceReads: the arena of the reads with keep[i] != 0 (reference id = rank among the kept reads)."""
        assert keep.dtype == torch.uint8 and keep.numel() == reads.n_reads
        h = N._P()
        _check(self, self.lib.cl_reads_select(self.h, reads.h, keep.contiguous().data_ptr(), C.byref(h)))
        return Reads(self, h)

    def reads_from_arena(self, packed: torch.Tensor, inv: torch.Tensor, lens: torch.Tensor) -> "Reads":
        """Arena from already packed words (word-aligned reads back to back), e.g. gathered from all ranks."""
        h = N._P()
        n = lens.numel()
        _check(self, self.lib.cl_reads_from_arena(self.h, packed.contiguous().data_ptr() if n else None, inv.contiguous().data_ptr() if n else None,
                                                  lens.contiguous().data_ptr() if n else None, n, C.byref(h)))
        return Reads(self, h)

    def pack_readset(self, rs) -> "Reads":
        return self.pack_reads(torch.from_numpy(rs.bases), torch.from_numpy(rs.offsets))

    # ---- a1 ----
    def kmer_scan(self, reads: "Reads", k: int, f: int, cap: int | None = None) -> torch.Tensor:
        if cap is None:
            cap = int(reads.total_bases // max(f, 1) * 1.3) + 4096 if f > 1 else int(reads.total_bases) + 64
        while True:
            out = torch.empty(cap, dtype=torch.int64, device=self.device)
            n = C.c_uint64(0)
            st = self.lib.cl_kmer_scan(self.h, reads.h, k, f, out.data_ptr(), cap, C.byref(n))
            if st == N.CL_E_CAPACITY:
                cap = int(n.value)
                continue
            _check(self, st)
            return out[:n.value]

    # ---- a2 + a3 ----
    def count_filter(self, kmers: torch.Tensor, k: int, ci: int, cs: int):
        kmers = kmers.contiguous()
        h = N._P()
        st = N.KmerStats()
        _check(self, self.lib.cl_kmer_count_filter(self.h, kmers.data_ptr(), kmers.numel(), k, ci, cs, C.byref(h), C.byref(st)))
        return KmerSet(self, h), st

    def kmer_set_from_keys(self, keys: torch.Tensor, counts: torch.Tensor, k: int) -> "KmerSet":
        """Replicated set from gathered per-rank partitions: sort by key on device, then build the table."""
        keys = keys.contiguous().clone()
        idx = torch.arange(keys.numel(), dtype=torch.int32, device=self.device)
        self.sort_u64(keys, idx, 0, 2 * k)
        counts = counts.contiguous()[idx.long()].contiguous()
        h = N._P()
        _check(self, self.lib.cl_kmer_set_create(self.h, keys.data_ptr(), counts.data_ptr(), keys.numel(), k, C.byref(h)))
        return KmerSet(self, h)

    # ---- a4 ----
    def accepted_kmers(self, kset: "KmerSet", reads: "Reads", k: int, f: int) -> "KmerLists":
        h = N._P()
        _check(self, self.lib.cl_accepted_kmers(self.h, kset.h, reads.h, k, f, C.byref(h)))
        return KmerLists(self, h)

    # ---- a6 ----
    def ref_accept(self, n_reads: int, n_pseudo: int, rng: int, exponent: float) -> np.ndarray:
        out = np.zeros(n_reads + n_pseudo, np.uint8)
        st = self.lib.cl_ref_accept(n_reads, n_pseudo, rng, exponent, out.ctypes.data)
        _check(self, st)
        return out

    # ---- a5 ----
    def index_build(self, kset, lists, accept: torch.Tensor, n_pseudo: int, max_kmer_count: int) -> "Index":
        accept = accept.to(self.device).contiguous()
        assert accept.dtype == torch.uint8 and accept.numel() == lists.n_reads
        h = N._P()
        _check(self, self.lib.cl_index_build(self.h, kset.h, lists.h, accept.data_ptr(), n_pseudo, max_kmer_count, C.byref(h)))
        return Index(self, h)

    def index_entries(self, lists, accept: torch.Tensor, ref_base: int):
        accept = accept.to(self.device).contiguous()
        bounds = torch.empty(lists.n_reads + 1, dtype=torch.int32, device=self.device)
        n, nacc = C.c_uint64(0), C.c_uint32(0)
        st = self.lib.cl_index_entries_of(self.h, lists.h, accept.data_ptr(), ref_base, None, None, 0, C.byref(n), bounds.data_ptr(), C.byref(nacc))
        if st not in (N.CL_OK, N.CL_E_CAPACITY):
            _check(self, st)
        ids = torch.empty(max(1, n.value), dtype=torch.int32, device=self.device)
        refs = torch.empty(max(1, n.value), dtype=torch.int32, device=self.device)
        if n.value:
            _check(self, self.lib.cl_index_entries_of(self.h, lists.h, accept.data_ptr(), ref_base, ids.data_ptr(), refs.data_ptr(), n.value, C.byref(n), None, None))
        return ids[:n.value], refs[:n.value], bounds, nacc.value

    def index_build_pairs(self, kset, ids, refs, bounds, n_refs_total: int, n_pseudo: int, max_kmer_count: int) -> "Index":
        ids, refs = ids.contiguous().clone(), refs.contiguous().clone()
        h = N._P()
        _check(self, self.lib.cl_index_build_pairs(self.h, kset.h, ids.data_ptr(), refs.data_ptr(), ids.numel(), bounds.data_ptr(),
                                                   bounds.numel() - 1, n_refs_total, n_pseudo, max_kmer_count, C.byref(h)))
        return Index(self, h)

    def candidates(self, index, lists, c: int):
        n = lists.n_reads
        refs = torch.empty((n, c), dtype=torch.int32, device=self.device)
        votes = torch.empty((n, c), dtype=torch.int32, device=self.device)
        cnt = torch.empty(n, dtype=torch.int32, device=self.device)
        _check(self, self.lib.cl_candidates(self.h, index.h, lists.h, c, refs.data_ptr(), votes.data_ptr(), cnt.data_ptr()))
        return refs, votes, cnt

    def candidates_at(self, index, lists, bounds: torch.Tensor, c: int):
        """The query of one chunk of reads against an index over the whole input: bounds[i] = reference reads before read i of `lists`."""
        n = lists.n_reads
        bounds = bounds.to(self.device).contiguous()
        assert bounds.dtype == torch.int32 and bounds.numel() == n + 1
        refs = torch.empty((n, c), dtype=torch.int32, device=self.device)
        votes = torch.empty((n, c), dtype=torch.int32, device=self.device)
        cnt = torch.empty(n, dtype=torch.int32, device=self.device)
        _check(self, self.lib.cl_candidates_at(self.h, index.h, lists.h, bounds.data_ptr(), c, refs.data_ptr(), votes.data_ptr(), cnt.data_ptr()))
        return refs, votes, cnt

    def candidates_common(self, index, lists, c: int, refs, cnt):
        n = lists.n_reads
        off = torch.empty(n * c + 1, dtype=torch.int64, device=self.device)
        need = C.c_uint64(0)
        st = self.lib.cl_candidates_common(self.h, index.h, lists.h, c, refs.data_ptr(), cnt.data_ptr(), off.data_ptr(), None, 0, C.byref(need))
        if st not in (N.CL_OK, N.CL_E_CAPACITY):
            _check(self, st)
        common = torch.empty(max(1, need.value), dtype=torch.int64, device=self.device)
        _check(self, self.lib.cl_candidates_common(self.h, index.h, lists.h, c, refs.data_ptr(), cnt.data_ptr(), off.data_ptr(),
                                                   common.data_ptr(), need.value, C.byref(need)))
        return off, common[:need.value]

    # ---- a13 + a15 ----
    def qual_coder(self, mode: int, source: int, level: int, fwd=(), rev=()) -> "QualCoder":
        prm = N.QualParams()
        prm.mode, prm.source, prm.level = mode, source, level
        prm.n_fwd, prm.n_rev = len(fwd), len(rev)
        for i, v in enumerate(fwd):
            prm.fwd[i] = v
        for i, v in enumerate(rev):
            prm.rev[i] = v
        h = N._P()
        _check(self, self.lib.cl_qual_coder_create(self.h, C.byref(prm), C.byref(h)))
        return QualCoder(self, h)

    def qual_decode_domains(self, mode: int, source: int, level: int, fwd, rev, reads: "Reads", payload: torch.Tensor, part_bounds, part_sizes, domain_first_part,
                            qual_off: torch.Tensor, flags: torch.Tensor | None = None, max_domains_per_launch: int = 0, want_symbols: bool = False):
        """cl_qual_decode_domains: the `qual` parts of whole model domains decoded on the device, one lane per domain.  Returns the ASCII
        qualities (a tensor of qual_off[-1] bytes) and, with want_symbols, (symbols, their n_reads + 1 offsets as a numpy array) for
        cl_digest_bytes_host(kind 2).  A part that does not decode raises ColordHipError(CL_E_MISMATCH) — with the qualities of the
        other domains in its `.quals`."""
        prm = N.QualParams()
        prm.mode, prm.source, prm.level = mode, source, level
        prm.n_fwd, prm.n_rev = len(fwd), len(rev)
        for i, v in enumerate(fwd):
            prm.fwd[i] = v
        for i, v in enumerate(rev):
            prm.rev[i] = v
        pb = np.ascontiguousarray(part_bounds, dtype=np.uint32)
        ps = np.ascontiguousarray(part_sizes, dtype=np.uint64)
        dom = np.ascontiguousarray(domain_first_part, dtype=np.uint32)
        qual_off, payload = qual_off.contiguous(), payload.contiguous()
        h_off = qual_off.cpu().numpy().astype(np.int64)
        n_reads = len(h_off) - 1
        navg = {1: 10, 2: 8, 3: 4, 7: 2}.get(mode, 0)
        per_base = mode <= 6
        sym_off = np.arange(n_reads + 1, dtype=np.int64) * navg + (h_off if per_base else 0)
        quals = torch.zeros(max(1, int(h_off[-1])), dtype=torch.uint8, device=self.device)
        syms = torch.zeros(max(1, int(sym_off[-1])), dtype=torch.uint8, device=self.device) if want_symbols else None
        st = self.lib.cl_qual_decode_domains(self.h, C.byref(prm), reads.h, None if flags is None else flags.data_ptr(), payload.data_ptr() if payload.numel() else None, payload.numel(),
                                             pb.ctypes.data, ps.ctypes.data, len(pb) - 1, dom.ctypes.data, len(dom), max_domains_per_launch,
                                             quals.data_ptr(), qual_off.data_ptr(), int(h_off[-1]), None if syms is None else syms.data_ptr(), 0 if syms is None else int(sym_off[-1]))
        try:
            _check(self, st)
        except N.ColordHipError as e:
            e.quals = quals[:int(h_off[-1])]
            raise
        if want_symbols:
            return quals[:int(h_off[-1])], (syms[:int(sym_off[-1])], sym_off.astype(np.uint64))
        return quals[:int(h_off[-1])]

    # ---- a8 ----
    def anchor_candidates(self, reads: "Reads", refs: "Reads", cand_refs: torch.Tensor, cand_n: torch.Tensor, anchor_len: int,
                          frac_always=0.9, frac_min=0.5, max_matches_mult=10.0, min_anchors=1, hifi=None) -> "Anchors":
        """hifi = (kmer_len, modulo, common_off, common) from candidates_common: HiFi k-mer anchors first (a9)."""
        c = cand_refs.shape[1]
        h = N._P()
        if hifi is not None:
            k, f, coff, common = hifi
            _check(self, self.lib.cl_anchor_candidates_hifi(self.h, reads.h, refs.h, cand_refs.contiguous().data_ptr(), cand_n.contiguous().data_ptr(), c, anchor_len,
                                                            frac_always, frac_min, max_matches_mult, min_anchors, k, f, coff.contiguous().data_ptr(),
                                                            common.contiguous().data_ptr() if common.numel() else None, C.byref(h)))
            return Anchors(self, h, reads.n_reads, c)
        _check(self, self.lib.cl_anchor_candidates(self.h, reads.h, refs.h, cand_refs.contiguous().data_ptr(), cand_n.contiguous().data_ptr(), c, anchor_len,
                                                   frac_always, frac_min, max_matches_mult, min_anchors, C.byref(h)))
        return Anchors(self, h, reads.n_reads, c)

    # ---- a12 (plain forms) ----
    def encode_plain(self, reads: "Reads"):
        n = reads.n_reads
        cap = int(reads.total_bases) + n
        es = torch.empty(max(cap, 1), dtype=torch.uint8, device=self.device)
        off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        nt = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        need = C.c_uint64(0)
        _check(self, self.lib.cl_encode_plain(self.h, reads.h, es.data_ptr(), cap, off.data_ptr(), nt.data_ptr(), C.byref(need)))
        return es[:need.value], off, nt[:n]

    # ---- a10-a12 ----
    def encode_reads(self, reads: "Reads", refs: "Reads", anchors: "Anchors", anchor_len: int, min_part_alt: int, max_rec: int, cost_mult: float,
                     pack_bounds=None):
        """CEncoder::Encode over the arena: returns (tuple bytes, byte offsets [n+1], tuple counts [n])."""
        import numpy as np
        n = reads.n_reads
        pb = np.ascontiguousarray(np.asarray([0, n] if pack_bounds is None else pack_bounds, dtype=np.uint32))
        off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        nt = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        need = C.c_uint64(0)
        cap = int(reads.total_bases) + 16 * n + 4096       # a stream never exceeds the plain form (1 B per base + header) by more than its headers
        for _ in range(2):
            es = torch.empty(max(cap, 1), dtype=torch.uint8, device=self.device)
            st = self.lib.cl_encode_reads(self.h, reads.h, refs.h, anchors.h, anchors.c, anchor_len, min_part_alt, max_rec, cost_mult,
                                          pb.ctypes.data, len(pb) - 1, es.data_ptr(), cap, off.data_ptr(), nt.data_ptr(), C.byref(need))
            if st == N.CL_E_CAPACITY and need.value > cap:
                cap = need.value
                continue
            _check(self, st)
            break
        return es[:need.value], off, nt[:n]

    def es_flags(self, reads: "Reads", es: torch.Tensor, es_off: torch.Tensor, base_off: torch.Tensor) -> torch.Tensor:
        """Per-base classes for the quality coder at levels 2-3 (quality_coder_impl.cpp:25-75) from the tuple streams."""
        flags = torch.empty(max(int(reads.total_bases), 1), dtype=torch.uint8, device=self.device)
        _check(self, self.lib.cl_es_flags(self.h, reads.h, es.contiguous().data_ptr() if es.numel() else None, es_off.contiguous().data_ptr(),
                                          base_off.contiguous().data_ptr(), flags.data_ptr()))
        return flags[:int(reads.total_bases)]

    # ---- the inverse of a10-a12 ----
    def es_expand(self, refs: "Reads", es: torch.Tensor, es_off: torch.Tensor, es_ntuples: torch.Tensor | None = None):
        """cl_es_expand: the reads their tuple streams describe against `refs`.  Returns (base codes 0..4, offsets [n+1])."""
        es, es_off = es.contiguous(), es_off.contiguous()
        n = es_off.numel() - 1
        nt = es_ntuples.contiguous() if es_ntuples is not None else None
        off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        need, codes, cap = C.c_uint64(0), None, 0
        for _ in range(2):
            st = self.lib.cl_es_expand(self.h, refs.h, es.data_ptr() if es.numel() else None, es_off.data_ptr(), nt.data_ptr() if nt is not None else None, n,
                                       codes.data_ptr() if codes is not None else None, cap, off.data_ptr(), C.byref(need))
            if st == N.CL_E_CAPACITY and need.value > cap:
                cap = need.value
                codes = torch.empty(cap, dtype=torch.uint8, device=self.device)
                continue
            _check(self, st)
            break
        return (codes[:need.value] if codes is not None else torch.empty(0, dtype=torch.uint8, device=self.device)), off

    def es_verify(self, reads: "Reads", refs: "Reads", es: torch.Tensor, es_off: torch.Tensor, es_ntuples: torch.Tensor | None = None):
        """cl_es_verify: (number of reads of `reads` that their tuple streams do not rebuild, the first of them or None)."""
        es, es_off = es.contiguous(), es_off.contiguous()
        nt = es_ntuples.contiguous() if es_ntuples is not None else None
        n_bad, first = C.c_uint64(0), C.c_uint32(0)
        _check(self, self.lib.cl_es_verify(self.h, reads.h, refs.h, es.data_ptr() if es.numel() else None, es_off.data_ptr(), nt.data_ptr() if nt is not None else None,
                                           C.byref(n_bad), C.byref(first)))
        return n_bad.value, (first.value if n_bad.value else None)

    def estimator_logs(self, count: torch.Tensor, total: torch.Tensor) -> torch.Tensor:
        """The decision logarithm -log2(count * (1/total)) as the encoder's kernels evaluate it (calc_logs, utils.h:800-810)."""
        count, total = count.contiguous(), total.contiguous()
        assert count.dtype == torch.int32 and total.dtype == torch.int32 and count.numel() == total.numel()
        out = torch.empty(count.numel(), dtype=torch.float64, device=self.device)
        _check(self, self.lib.cl_estimator_logs(self.h, count.data_ptr(), total.data_ptr(), count.numel(), out.data_ptr()))
        return out

    # ---- the whole data path of one shard in one native call ----
    def compress_shard(self, reads: "Reads", params: dict, part_bounds, pack_bounds, dna: "DnaCoder", qual: "QualCoder | None" = None,
                       quals: torch.Tensor | None = None, base_off: torch.Tensor | None = None):
        """cl_compress_shard: returns (dna payload, dna part sizes, qual payload or None, qual part sizes, info dict)."""
        import numpy as np
        P = N.CompressParams()
        for k_, v in params.items():
            setattr(P, k_, v)
        pb = np.ascontiguousarray(np.asarray(part_bounds, dtype=np.uint32)); kb = np.ascontiguousarray(np.asarray(pack_bounds, dtype=np.uint32))
        npart = len(pb) - 1
        dcap = int(reads.total_bases) + 64 * npart + 4096
        dout = torch.empty(dcap, dtype=torch.uint8, device=self.device)
        dsz = np.zeros(max(npart, 1), np.uint64)
        qout, qsz, qcap = None, np.zeros(max(npart, 1), np.uint64), 0
        if qual is not None:
            qcap = int(int(reads.total_bases) * 1.35) + 64 * npart + 4096
            qout = torch.empty(qcap, dtype=torch.uint8, device=self.device)
        info = N.CompressInfo()
        _check(self, self.lib.cl_compress_shard(self.h, C.byref(P), reads.h, quals.data_ptr() if qual is not None else None,
                                                base_off.contiguous().data_ptr() if qual is not None else None,
                                                pb.ctypes.data, npart, kb.ctypes.data, len(kb) - 1, dna.h, qual.h if qual is not None else None,
                                                dout.data_ptr(), dcap, dsz.ctypes.data, qout.data_ptr() if qout is not None else None, qcap, qsz.ctypes.data, C.byref(info)))
        if qual is not None and qual.ctx is not self:
            _check(qual.ctx, N.CL_OK)                       # collect the kernel times of the concurrent quality stream
        inf = {n_: getattr(info, n_) for n_, _ in N.CompressInfo._fields_ if n_ != "pad"}
        return dout[:inf["dna_bytes"]], dsz[:npart], (qout[:inf["qual_bytes"]] if qout is not None else None), qsz[:npart], inf

    # ---- the same path chunk by chunk (any input size; one rank of a multi-GPU run when `exchange` is given) ----
    def compressor(self, params: dict, qual_params=None, qual_ctx: "Context | None" = None, exchange=None, expected_bases: int = 0) -> "Compressor":
        """cl_compressor_create.  qual_params: (mode, source, level, fwd, rev) or None."""
        P = N.CompressParams()
        for k_, v in params.items():
            setattr(P, k_, v)
        Q = None
        if qual_params is not None:
            mode, source, level, fwd, rev = qual_params
            Q = N.QualParams(mode=mode, source=source, level=level, n_fwd=len(fwd), n_rev=len(rev))
            for i, v in enumerate(fwd):
                Q.fwd[i] = v
            for i, v in enumerate(rev):
                Q.rev[i] = v
        h = N._P()
        _check(self, self.lib.cl_compressor_create(self.h, qual_ctx.h if qual_ctx is not None else None, C.byref(P), C.byref(Q) if Q is not None else None,
                                                   C.byref(exchange.c_struct) if exchange is not None else None, int(expected_bases), C.byref(h)))
        return Compressor(self, h, qual_ctx, Q is not None, exchange)

    # ---- a14 ----
    def dna_coder(self, max_alt_refs: int, level: int, start_read_id: int = 0) -> "DnaCoder":
        h = N._P()
        _check(self, self.lib.cl_dna_coder_create(self.h, max_alt_refs, level, start_read_id, C.byref(h)))
        return DnaCoder(self, h, max_alt_refs)

    def sort_u64(self, keys: torch.Tensor, vals: torch.Tensor | None = None, begin_bit=0, end_bit=64):
        if vals is None:
            _check(self, self.lib.cl_sort_u64(self.h, keys.data_ptr(), keys.numel(), begin_bit, end_bit))
        else:
            _check(self, self.lib.cl_sort_u64_u32(self.h, keys.data_ptr(), vals.data_ptr(), keys.numel(), begin_bit, end_bit))

    # ---- the device primitives alone (csrc/scan.hip, csrc/sort.hip): int32 / int64 tensors carry uint32 / uint64 bit patterns ----
    def sort_u32(self, keys: torch.Tensor, vals: torch.Tensor | None = None, begin_bit=0, end_bit=32):
        assert keys.dtype == torch.int32 and (vals is None or vals.dtype == torch.int32)
        if vals is None:
            _check(self, self.lib.cl_sort_u32(self.h, keys.data_ptr(), keys.numel(), begin_bit, end_bit))
        else:
            _check(self, self.lib.cl_sort_u32_u32(self.h, keys.data_ptr(), vals.data_ptr(), keys.numel(), begin_bit, end_bit))

    def sort_swap(self, keys: torch.Tensor, vals: torch.Tensor, begin_bit, end_bit):
        """The coders' form of the sort (buffers that may be swapped with the temporaries): -> (sorted keys, their values); the inputs stay."""
        assert keys.dtype in (torch.int32, torch.int64) and vals.dtype == torch.int32 and vals.numel() == keys.numel()
        ko, vo = torch.empty_like(keys), torch.empty_like(vals)
        f = self.lib.cl_sort_swap_u32_u32 if keys.dtype == torch.int32 else self.lib.cl_sort_swap_u64_u32
        _check(self, f(self.h, keys.data_ptr(), vals.data_ptr(), keys.numel(), begin_bit, end_bit, ko.data_ptr(), vo.data_ptr()))
        return ko, vo

    def scan_u32(self, data: torch.Tensor, want_total: bool = True):
        """In-place exclusive prefix sums of uint32 -> the total (None if not asked for: then a sum beyond 32 bits is not refused)."""
        assert data.dtype == torch.int32
        total = C.c_uint64(0)
        _check(self, self.lib.cl_scan_u32(self.h, data.data_ptr(), data.numel(), C.byref(total) if want_total else None))
        return total.value if want_total else None

    def scan_u32_u64(self, data: torch.Tensor, out: torch.Tensor, want_total: bool = True):
        """out[0 .. n] = exclusive prefix sums of the uint32 in data, in 64 bits; out[n] = the total, returned too if asked for."""
        assert data.dtype == torch.int32 and out.dtype == torch.int64 and out.numel() == data.numel() + 1
        total = C.c_uint64(0)
        _check(self, self.lib.cl_scan_u32_u64(self.h, data.data_ptr(), out.data_ptr(), data.numel(), C.byref(total) if want_total else None))
        return total.value if want_total else None

    def run_starts(self, keys: torch.Tensor, shift: int, seg: torch.Tensor) -> int:
        """seg[0 .. r] = starts of the runs of equal key >> shift in sorted keys, then n; -> r.  seg must have room for r + 1."""
        assert keys.dtype in (torch.int32, torch.int64) and seg.dtype == torch.int32
        f = self.lib.cl_run_starts_u32 if keys.dtype == torch.int32 else self.lib.cl_run_starts_u64
        r = C.c_uint64(0)
        _check(self, f(self.h, keys.data_ptr(), keys.numel(), shift, seg.data_ptr(), seg.numel(), C.byref(r)))
        return r.value


class _Obj:
    _free = None

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def free(self):
        if self.h:
            getattr(self.ctx.lib, self._free)(self.h)
            self.h = None

    def _arr(self, getter, n, dtype):
        ptr = getattr(self.ctx.lib, getter)(self.h)
        return _view(ptr, n, dtype, self.ctx.device)


class Pileup(_Obj):
    """cl_pileup: per-position base counts of the reads aligned to a reference genome's pieces (csrc/pileup.hip)."""
    _free = "cl_pileup_free"
    SITE_FIELDS = ("seq", "pos", "ref", "kind", "match", "subA", "subC", "subG", "subT", "del", "ins", "depth")
    COLUMNS = ("match", "subA", "subC", "subG", "subT", "del", "ins", "ref")

    def __init__(self, ctx, h, owned=True):
        super().__init__(ctx, h)
        self.owned = owned

    def free(self):
        if self.owned:
            super().free()
        self.h = None

    @property
    def n_pos(self): return self.ctx.lib.cl_pileup_positions(self.h)

    def add(self, refs: "Reads", es: torch.Tensor, es_off: torch.Tensor, max_blocks: int = 0):
        """cl_pileup_add: the tuple streams es / es_off (n + 1 byte offsets) against the arena the table was created for.  A malformed stream
        raises (CL_E_INVALID, the text names the first such read) and spoils the table."""
        es, es_off = es.contiguous(), es_off.contiguous()
        n = max(es_off.numel() - 1, 0)
        _check(self.ctx, self.ctx.lib.cl_pileup_add(self.h, refs.h, es.data_ptr() if n else None, es_off.data_ptr() if n else None, n, max_blocks))

    def finish(self):
        _check(self.ctx, self.ctx.lib.cl_pileup_finish(self.h))

    def columns(self, first: int = 0, n: "int | None" = None) -> np.ndarray:
        """cl_pileup_columns: (n, 8) uint32 — match, sub A C G T, del, ins, ref — of the positions first .. first + n - 1"""
        n = self.n_pos - first if n is None else n
        out = np.zeros((n, 8), np.uint32)
        _check(self.ctx, self.ctx.lib.cl_pileup_columns(self.h, first, n, out.ctypes.data if n else None))
        return out

    def sites(self, min_depth: int = 4, min_alt: int = 3, min_permille: int = 250, cap: "int | None" = None) -> np.ndarray:
        """cl_pileup_sites: (m, 12) uint32 in the field order of cl_pileup_site, in genome order.  With cap the call is made once with room for
        cap records (CL_E_CAPACITY raises); without, the need is asked for first."""
        need = C.c_uint64(0)
        args = (self.h, min_depth, min_alt, min_permille)
        if cap is None:
            st = self.ctx.lib.cl_pileup_sites(*args, None, 0, C.byref(need))
            if st not in (N.CL_OK, N.CL_E_CAPACITY):
                _check(self.ctx, st)
            cap = need.value
        out = np.zeros((cap, 12), np.uint32)
        _check(self.ctx, self.ctx.lib.cl_pileup_sites(*args, out.ctypes.data if cap else None, cap, C.byref(need)))
        return out[:need.value]

    def totals(self) -> dict:
        s = N.PileupSums()
        _check(self.ctx, self.ctx.lib.cl_pileup_totals(self.h, C.byref(s)))
        return s.as_dict()


class Reads(_Obj):
    _free = "cl_reads_free"

    @property
    def n_reads(self): return self.ctx.lib.cl_reads_count(self.h)
    @property
    def total_bases(self): return self.ctx.lib.cl_reads_total_bases(self.h)
    @property
    def total_words(self): return self.ctx.lib.cl_reads_total_words(self.h)
    def packed(self): return self._arr("cl_reads_packed", self.total_words + 1, torch.int64)
    def invalid(self): return self._arr("cl_reads_invalid", self.total_words + 1, torch.int32)
    def word_offsets(self): return self._arr("cl_reads_word_offsets", self.n_reads + 1, torch.int64)
    def lengths(self): return self._arr("cl_reads_lengths", self.n_reads, torch.int32)
    def has_n(self): return self._arr("cl_reads_has_n", self.n_reads, torch.uint8)

    def compact(self, i: int) -> bytes:
        buf = np.zeros(1 << 20, np.uint8)
        n = C.c_uint64(0)
        st = self.ctx.lib.cl_reads_compact(self.ctx.h, self.h, i, buf.ctypes.data, buf.size, C.byref(n))
        if st == N.CL_E_CAPACITY:
            buf = np.zeros(n.value, np.uint8)
            st = self.ctx.lib.cl_reads_compact(self.ctx.h, self.h, i, buf.ctypes.data, buf.size, C.byref(n))
        _check(self.ctx, st)
        return bytes(buf[:n.value])


class KmerSet(_Obj):
    _free = "cl_kmer_set_free"

    @property
    def size(self): return self.ctx.lib.cl_kmer_set_size(self.h)
    def keys(self): return self._arr("cl_kmer_set_keys", self.size, torch.int64)
    def counts(self): return self._arr("cl_kmer_set_counts", self.size, torch.int32)

    def check(self, kmers: torch.Tensor) -> torch.Tensor:
        out = torch.empty(kmers.numel(), dtype=torch.uint8, device=self.ctx.device)
        _check(self.ctx, self.ctx.lib.cl_kmer_set_check(self.ctx.h, self.h, kmers.data_ptr(), kmers.numel(), out.data_ptr()))
        return out


class KmerLists(_Obj):
    _free = "cl_kmer_lists_free"

    @property
    def n_reads(self): return self.ctx.lib.cl_kmer_lists_reads(self.h)
    @property
    def total(self): return self.ctx.lib.cl_kmer_lists_total(self.h)
    def offsets(self): return self._arr("cl_kmer_lists_offsets", self.n_reads + 1, torch.int64)
    def kmers(self): return self._arr("cl_kmer_lists_kmers", self.total, torch.int64)
    def ids(self): return self._arr("cl_kmer_lists_ids", self.total, torch.int32)
    def pos(self): return self._arr("cl_kmer_lists_pos", self.total, torch.int32)


class Index(_Obj):
    _free = "cl_index_free"

    @property
    def n_refs(self): return self.ctx.lib.cl_index_n_refs(self.h)
    @property
    def entries(self): return self.ctx.lib.cl_index_entries(self.h)


class QualCoder(_Obj):
    _free = "cl_qual_coder_free"

    def encode(self, reads: "Reads", quals: torch.Tensor, qual_off: torch.Tensor, part_bounds, flags: torch.Tensor | None = None):
        """Returns (payload bytes tensor on device, list of part sizes)."""
        ctx = self.ctx
        pb = np.ascontiguousarray(part_bounds, dtype=np.uint32)
        n_parts = len(pb) - 1
        sizes = np.zeros(max(n_parts, 1), np.uint64)
        cap = max(4096, int(quals.numel() * 1.35) + 64 * n_parts)     # generous: org mode on noisy data is ~1 B/base
        while True:
            out = torch.empty(cap, dtype=torch.uint8, device=ctx.device)
            n = C.c_uint64(0)
            st = ctx.lib.cl_qual_encode(ctx.h, self.h, reads.h, quals.data_ptr(), qual_off.data_ptr(),
                                        None if flags is None else flags.data_ptr(), pb.ctypes.data, n_parts,
                                        out.data_ptr(), cap, sizes.ctypes.data, C.byref(n))
            if st == N.CL_E_CAPACITY and n.value > cap:
                raise N.ColordHipError(st, "qual output capacity exceeded after models advanced; retry with a larger cap")
            _check(ctx, st)
            return out[:n.value], [int(x) for x in sizes[:n_parts]]

    def set_domain_symbols(self, n: int):
        """cl_qual_coder_set_domain_symbols: the models start afresh at the first part boundary at which the open domain holds n symbols (0: never)."""
        _check(self.ctx, self.ctx.lib.cl_qual_coder_set_domain_symbols(self.h, n))

    def domains(self) -> list:
        """cl_qual_coder_domains: the first part of every model domain so far, counted over the coder's lifetime."""
        return _domain_list(self.ctx, self.ctx.lib.cl_qual_coder_domains, self.h)

    def model(self, family: int, context: int) -> np.ndarray:
        """cl_qual_coder_model: the counters and, last, the total of one adaptive model after the last encode()."""
        out = np.zeros(257, np.uint32)
        n = C.c_uint32(0)
        _check(self.ctx, self.ctx.lib.cl_qual_coder_model(self.h, family, context, out.ctypes.data, len(out), C.byref(n)))
        return out[:n.value].copy()

    def groups(self) -> int:
        """cl_qual_coder_groups: the groups of parts taken through the model kernels so far."""
        n = C.c_uint64(0)
        _check(self.ctx, self.ctx.lib.cl_qual_coder_groups(self.h, C.byref(n)))
        return n.value


def _domain_list(ctx, fn, h):
    n = C.c_uint64(0)
    st = fn(h, None, 0, C.byref(n))
    if st not in (N.CL_OK, N.CL_E_CAPACITY):
        _check(ctx, st)
    out = np.zeros(max(1, n.value), np.uint64)
    _check(ctx, fn(h, out.ctypes.data, out.size, C.byref(n)))
    return [int(x) for x in out[:n.value]]


def _overlap_records(fn, h) -> np.ndarray:
    """the records a context or a compressor keeps (cl_ctx_overlaps / cl_compressor_overlaps): the need first, then that many"""
    n = C.c_uint64(0)
    st = fn(h, None, 0, C.byref(n))
    if st not in (N.CL_OK, N.CL_E_CAPACITY):
        _check(None, st)
    out = np.zeros((n.value, 12), np.uint32)
    if n.value:
        _check(None, fn(h, out.ctypes.data, n.value, C.byref(n)))
    return out[:n.value]


def _cigar_records(fn, h):
    """the CIGARs a context or a compressor keeps (cl_ctx_cigars / cl_compressor_cigars): the needs first, then that many"""
    nr, no = C.c_uint64(0), C.c_uint64(0)
    st = fn(h, None, 0, C.byref(nr), None, 0, C.byref(no))
    if st not in (N.CL_OK, N.CL_E_CAPACITY):
        _check(None, st)
    rec, ops = np.zeros(nr.value, np.uint32), np.zeros(no.value, np.uint32)
    if nr.value:
        _check(None, fn(h, rec.ctypes.data, nr.value, C.byref(nr), ops.ctypes.data if no.value else None, no.value, C.byref(no)))
    return rec[:nr.value], ops[:no.value]


def _cigar_coded(fn, h):
    """the coded CIGARs a context or a compressor keeps (cl_ctx_cigars_coded / cl_compressor_cigars_coded): the needs first, then that many"""
    nr, nb, no, ns = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    st = fn(h, None, 0, C.byref(nr), None, 0, C.byref(nb), C.byref(no), C.byref(ns))
    if st not in (N.CL_OK, N.CL_E_CAPACITY):
        _check(None, st)
    rec, raw = np.zeros(nr.value, np.uint32), np.zeros(max(nb.value, 1), np.uint8)
    if nr.value or nb.value:
        _check(None, fn(h, rec.ctypes.data if nr.value else None, nr.value, C.byref(nr), raw.ctypes.data, nb.value, C.byref(nb), C.byref(no), C.byref(ns)))
    return rec[:nr.value], raw[:nb.value].tobytes(), no.value, ns.value


def cigars_pack_host(words, part_ops: int = 0, seg_ops: int = 0) -> bytes:
    """cl_cigars_pack_host: the coded segments of the operation words, by the host twin; ValueError names the first word that is no operation"""
    lib = N.load()
    w = np.ascontiguousarray(words, dtype=np.uint32)
    nb, bad = C.c_uint64(0), C.c_uint64(0)
    st = lib.cl_cigars_pack_host(w.ctypes.data if w.size else None, w.size, part_ops, seg_ops, None, 0, C.byref(nb), C.byref(bad))
    if st == N.CL_E_INVALID:
        raise ValueError("cl_cigars_pack_host: word %d is no operation" % bad.value if bad.value != 2 ** 64 - 1 else "cl_cigars_pack_host: a knob out of range")
    out = np.zeros(max(nb.value, 1), np.uint8)
    st = lib.cl_cigars_pack_host(w.ctypes.data if w.size else None, w.size, part_ops, seg_ops, out.ctypes.data, nb.value, C.byref(nb), C.byref(bad))
    assert st == N.CL_OK, st
    return out[:nb.value].tobytes()


def cigars_unpack_host(data: bytes) -> np.ndarray:
    """cl_cigars_unpack_host: the operation words of coded segments; ValueError with the reason (cl_cigars_check_host) when they are refused"""
    lib = N.load()
    raw = np.frombuffer(data, np.uint8)
    no = C.c_uint64(0)
    st = lib.cl_cigars_unpack_host(raw.ctypes.data if raw.size else None, raw.size, None, 0, C.byref(no))
    if st == N.CL_E_INVALID:
        raise ValueError(lib.cl_cigars_refusal(lib.cl_cigars_check_host(raw.ctypes.data if raw.size else None, raw.size)).decode())
    out = np.zeros(max(no.value, 1), np.uint32)
    st = lib.cl_cigars_unpack_host(raw.ctypes.data if raw.size else None, raw.size, out.ctypes.data, no.value, C.byref(no))
    assert st == N.CL_OK, st
    return out[:no.value].copy()


class Compressor(_Obj):
    """cl_compressor: pass 1 / reference listing / pass 2 over the chunks of an input (csrc/stream.hip)."""
    _free = "cl_compressor_free"

    def cigars_coded(self):
        """cl_compressor_cigars_coded: the record counts and the coded segments of the CIGARs (Context.set_cigars_coded)."""
        return _cigar_coded(self.ctx.lib.cl_compressor_cigars_coded, self.h)

    def cigars(self):
        """cl_compressor_cigars: the CIGARs of the records of mappings() (Context.set_cigars), in their order."""
        return _cigar_records(self.ctx.lib.cl_compressor_cigars, self.h)

    def overlaps(self) -> np.ndarray:
        """cl_compressor_overlaps: the overlap records of the chunks whose tuple streams are made (Context.set_overlaps), in input order."""
        return _overlap_records(self.ctx.lib.cl_compressor_overlaps, self.h)

    def __init__(self, ctx, h, qual_ctx, has_qual, exchange):
        super().__init__(ctx, h)
        self.qual_ctx, self.has_qual, self.exchange = qual_ctx, has_qual, exchange       # (the exchange's callbacks must outlive the handle)

    def count_add(self, reads: "Reads"):
        _check(self.ctx, self.ctx.lib.cl_compressor_count_add(self.h, reads.h))

    def count_finish(self):
        st = N.KmerStats()
        _check(self.ctx, self.ctx.lib.cl_compressor_count_finish(self.h, C.byref(st)))
        return st

    def refs_add(self, reads: "Reads"):
        _check(self.ctx, self.ctx.lib.cl_compressor_refs_add(self.h, reads.h))

    def refs_finish(self):
        _check(self.ctx, self.ctx.lib.cl_compressor_refs_finish(self.h))

    def info(self) -> dict:
        st = N.KmerStats(); a, b, m = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0); r, nr = C.c_uint32(0), C.c_uint32(0)
        _check(self.ctx, self.ctx.lib.cl_compressor_info(self.h, C.byref(st), C.byref(a), C.byref(b), C.byref(m), C.byref(r), C.byref(nr)))
        return dict(tot_kmers=st.tot_kmers, n_unique_counted=st.n_unique_counted, first_read=a.value, n_reads_total=b.value, mean_read_len=m.value,
                    sparse_range=r.value, n_refs_total=nr.value)

    def verified(self):
        """cl_compressor_verified: (reads, bases) rebuilt from their edit scripts and compared with the input (Context.set_verify)."""
        r, b = C.c_uint64(0), C.c_uint64(0)
        _check(None, self.ctx.lib.cl_compressor_verified(self.h, C.byref(r), C.byref(b)))
        return r.value, b.value

    def verified_streams(self):
        """cl_compressor_verified_streams: (parts, symbols, bytes) of the dna and qual streams decoded against their models' intervals
        (Context.set_verify_streams), over the compressor's context and its quality coder's."""
        p, s, b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(None, self.ctx.lib.cl_compressor_verified_streams(self.h, C.byref(p), C.byref(s), C.byref(b)))
        return p.value, s.value, b.value

    def digest(self):
        """cl_compressor_digest: ((reads, symbols, sum) dna, the same qual) of the chunks encoded so far (Context.set_digest)."""
        d, q = N.Digest(), N.Digest()
        _check(None, self.ctx.lib.cl_compressor_digest(self.h, C.byref(d), C.byref(q)))
        return d.triple(), q.triple()

    def edit_profile(self) -> "N.Edits":
        """cl_compressor_edit_profile: the edit-operation profile of the chunks whose tuple streams are made (Context.set_edit_profile)."""
        e = N.Edits()
        _check(None, self.ctx.lib.cl_compressor_edit_profile(self.h, C.byref(e)))
        return e

    def report(self) -> "N.Report":
        """cl_compressor_report: the content report of the chunks encoded so far (Context.set_report)."""
        r = N.Report()
        _check(None, self.ctx.lib.cl_compressor_report(self.h, C.byref(r)))
        return r

    def digest_values(self):
        """cl_compressor_digest_values: (reads, symbols, sum) of the qual-values digest of the chunks encoded so far (Context.set_digest_values)."""
        d = N.Digest()
        _check(None, self.ctx.lib.cl_compressor_digest_values(self.h, C.byref(d)))
        return d.triple()

    def set_qual_domain_symbols(self, n: int):
        """cl_compressor_set_qual_domain_symbols: model domains of the quality stream; before the first encode / prepare call."""
        _check(self.ctx, self.ctx.lib.cl_compressor_set_qual_domain_symbols(self.h, n))

    def qual_domains(self) -> list:
        """cl_compressor_qual_domains: the first `qual` part of every model domain so far."""
        return _domain_list(self.ctx, self.ctx.lib.cl_compressor_qual_domains, self.h)

    def genome_add(self, sequences: "Reads"):
        _check(self.ctx, self.ctx.lib.cl_compressor_genome_add(self.h, sequences.h))

    def pseudo_reads(self, pseudo: "Reads"):
        _check(self.ctx, self.ctx.lib.cl_compressor_pseudo_reads(self.h, pseudo.h))

    def genome_geometry(self, seq_len, read_len: int, overlap: int):
        """cl_compressor_genome_geometry: the geometry the pseudo reads were cut by (Context.set_mappings lifts with it); one that does not
        give exactly the pseudo reads raises (CL_E_INVALID)."""
        sl = np.ascontiguousarray(np.asarray(seq_len, dtype=np.uint64))
        _check(self.ctx, self.ctx.lib.cl_compressor_genome_geometry(self.h, sl.ctypes.data if len(sl) else None, len(sl), read_len, overlap))

    def mappings(self) -> np.ndarray:
        """cl_compressor_mappings: the lifted records of the chunks whose tuple streams are made (Context.set_mappings), in input order."""
        return _overlap_records(self.ctx.lib.cl_compressor_mappings, self.h)

    def pileup(self) -> "Pileup":
        """cl_compressor_pileup: the compressor's table (Context.set_pileup), finished, after the last encode(); it goes with the compressor."""
        h = N._P()
        _check(self.ctx, self.ctx.lib.cl_compressor_pileup(self.h, C.byref(h)))
        return Pileup(self.ctx, h, owned=False)

    def prepare(self, reads: "Reads", pack_bounds, part_bounds=None, quals: torch.Tensor | None = None, base_off: torch.Tensor | None = None):
        """cl_compressor_prepare[_parts]: announce a chunk of a later encode() call; its candidates / anchors / edit scripts are
        computed in the background on an encode lane while the chunks before it are coded — and, with the part bounds of that
        encode() call, the model-independent half of its `dna` coding (walks, sort by context) on the preparation thread."""
        kb = np.ascontiguousarray(np.asarray(pack_bounds, dtype=np.uint32))
        if part_bounds is None:
            _check(self.ctx, self.ctx.lib.cl_compressor_prepare(self.h, reads.h, kb.ctypes.data, len(kb) - 1))
        else:
            pb = np.ascontiguousarray(np.asarray(part_bounds, dtype=np.uint32))
            _check(self.ctx, self.ctx.lib.cl_compressor_prepare_parts(self.h, reads.h, kb.ctypes.data, len(kb) - 1, pb.ctypes.data, len(pb) - 1,
                                                                      quals.data_ptr() if quals is not None else None, base_off.data_ptr() if (quals is not None and base_off is not None) else None))

    def encode(self, reads: "Reads", part_bounds, pack_bounds, quals: torch.Tensor | None = None, base_off: torch.Tensor | None = None,
               dna_out: torch.Tensor | None = None, qual_out: torch.Tensor | None = None):
        """One chunk of pass 2.  Returns (dna payload, dna part sizes, qual payload or None, qual part sizes, info dict); with
        dna_out / qual_out the payloads are written to the START of those caller tensors (views are returned)."""
        ctx = self.ctx
        pb = np.ascontiguousarray(np.asarray(part_bounds, dtype=np.uint32)); kb = np.ascontiguousarray(np.asarray(pack_bounds, dtype=np.uint32))
        npart = len(pb) - 1
        if dna_out is None:
            dna_out = torch.empty(int(reads.total_bases) + 64 * npart + 4096, dtype=torch.uint8, device=ctx.device)
        dsz, qsz = np.zeros(max(npart, 1), np.uint64), np.zeros(max(npart, 1), np.uint64)
        if self.has_qual and qual_out is None:
            qual_out = torch.empty(int(int(reads.total_bases) * 1.35) + 64 * npart + 4096, dtype=torch.uint8, device=ctx.device)
        info = N.CompressInfo()
        _check(ctx, ctx.lib.cl_compressor_encode(self.h, reads.h, quals.data_ptr() if self.has_qual else None, base_off.contiguous().data_ptr() if self.has_qual else None,
                                                 pb.ctypes.data, npart, kb.ctypes.data, len(kb) - 1, dna_out.data_ptr(), dna_out.numel(), dsz.ctypes.data,
                                                 qual_out.data_ptr() if self.has_qual else None, qual_out.numel() if self.has_qual else 0, qsz.ctypes.data, C.byref(info)))
        if self.qual_ctx is not None and self.qual_ctx is not ctx:
            _check(self.qual_ctx, N.CL_OK)                  # collect the kernel times of the concurrent quality stream
        inf = {n_: getattr(info, n_) for n_, _ in N.CompressInfo._fields_ if n_ != "pad"}
        return dna_out[:inf["dna_bytes"]], dsz[:npart], (qual_out[:inf["qual_bytes"]] if self.has_qual else None), qsz[:npart], inf


class DnaCoder(_Obj):
    _free = "cl_dna_coder_free"
    N_SYM = (3, 2, 2, 32, 256, 4, 5, 256, 0, 24, 256, 256, 8)          # symbols per model family (0: max_alt_refs)

    def __init__(self, ctx, h, max_alt_refs):
        super().__init__(ctx, h)
        self.max_alt_refs = max_alt_refs

    def encode(self, refs: "Reads", es: torch.Tensor, es_off: torch.Tensor, es_ntuples: torch.Tensor, part_bounds):
        """Returns (payload bytes tensor on device, list of part sizes)."""
        ctx = self.ctx
        pb = np.ascontiguousarray(part_bounds, dtype=np.uint32)
        n_parts = len(pb) - 1
        n_reads = es_off.numel() - 1
        sizes = np.zeros(max(n_parts, 1), np.uint64)
        cap = max(4096, int(es.numel() * 0.6) + 64 * n_parts)
        out = torch.empty(cap, dtype=torch.uint8, device=ctx.device)
        n = C.c_uint64(0)
        st = ctx.lib.cl_dna_encode(ctx.h, self.h, refs.h, es.data_ptr(), es_off.data_ptr(), es_ntuples.data_ptr(), n_reads,
                                   pb.ctypes.data, n_parts, out.data_ptr(), cap, sizes.ctypes.data, C.byref(n))
        _check(ctx, st)
        return out[:n.value], [int(x) for x in sizes[:n_parts]]

    def model(self, family: int, context: int) -> np.ndarray:
        """cl_dna_coder_model: the counters and, last, the total of one adaptive model after the last encode()."""
        out = np.zeros(257, np.uint32)
        _check(self.ctx, self.ctx.lib.cl_dna_coder_model(self.h, family, context, out.ctypes.data))
        return out[:(self.N_SYM[family] or self.max_alt_refs) + 1].copy()


class Anchors(_Obj):
    _free = "cl_anchors_free"

    def __init__(self, ctx, h, n_reads, c):
        super().__init__(ctx, h)
        self.n_reads, self.c = n_reads, c

    @property
    def total(self): return self.ctx.lib.cl_anchors_total(self.h)

    def lis_counts(self):
        """(tasks, pairs) chained by a wave and (tasks, pairs) chained by a lane, non-empty tasks only."""
        lib = self.ctx.lib
        return ((lib.cl_anchors_wave_tasks(self.h), lib.cl_anchors_wave_pairs(self.h)), (lib.cl_anchors_lane_tasks(self.h), lib.cl_anchors_lane_pairs(self.h)))

    def n_cands(self): return self._arr("cl_anchors_n_cands", self.n_reads, torch.int32)
    def cands(self): return self._arr("cl_anchors_cands", self.n_reads * self.c * 4, torch.int32).view(self.n_reads, self.c, 4)
    def cand_offsets(self): return self._arr("cl_anchors_cand_offsets", self.n_reads * self.c + 1, torch.int64)
    def data(self): return self._arr("cl_anchors_data", self.total * 3, torch.int32).view(-1, 3)
