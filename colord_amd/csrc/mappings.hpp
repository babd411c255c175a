// mappings.hpp — read-to-genome mappings of a reference-genome run.  With -G the genome is cut into overlapping pieces, the
// pseudo reads, which are reference ids 0 .. n_pseudo-1; every read is aligned against them like against any reference read.  An overlap
// record (overlaps.hpp) whose target is such an id is an alignment of the read against a PIECE of the genome; the LIFT moves it to the
// coordinates of the genome's sequence the piece was cut from.  On the device: k_map_lift (mappings.hip).  Here: the geometry of the
// pieces, the lift of one record — ONE function for the kernel and the host twin, so that the two cannot disagree — and the host twin.
//
// Geometry: n_seqs sequences of seq_len[s] bases (each below 2^32), pieces of read_len bases every step = read_len - overlap bases
// (genome_io::pseudo_reads): sequence s has ceil(seq_len[s] / step) pieces, the ids piece_first[s] .. piece_first[s + 1] - 1; piece p starts
// at (p - piece_first[s]) * step and is min(read_len, seq_len[s] - start) long.  A sequence of no bases has no piece.
//
// The lift of a record: t >= n_pseudo targets a read of the input and is DROPPED.  Otherwise s comes from a search in piece_first, ts and
// te grow by the piece's start, tlen becomes seq_len[s], t becomes s, flags gets OV_GENOME; every other field stays.  Refused, in this
// order: the record's tlen is not the piece's length; a lifted position past 2^32 - 1; te lifted past seq_len[s].
//
// Under a host compiler alone this header needs no HIP (tests/tools/mappings_host_test.cpp).
#pragma once
#include <vector>
#include "overlaps.hpp"

constexpr uint32_t OV_GENOME = 4;                                          // flags bit 2: t is a sequence of the genome, ts / te its coordinates
// what refuses a record (cl_mappings_lift_host's bad_code; map_error_text(code))
enum : uint32_t { MAPE_NONE = 0, MAPE_TLEN = 1, MAPE_POS = 2, MAPE_END = 3 };
inline const char* map_error_text(uint32_t code)
{
	static const char* const T[4] = { "no error", "the record's target length is not the length of its genome piece", "a lifted position past 2^32 - 1", "the lifted target end lies past the end of its sequence" };
	return code < 4 ? T[code] : "unknown code";
}

// seq_len: n_seqs entries; piece_first: n_seqs + 1 entries, piece_first[n_seqs] = n_pseudo (host or device pointers, as the caller runs)
struct MapGeom { const uint64_t* seq_len; const uint32_t* piece_first; uint32_t n_seqs, n_pseudo, read_len, step; };

// piece_first of a geometry (n_seqs + 1 entries).  CL_E_INVALID: read_len <= overlap, or sequences without their lengths; CL_E_UNSUPPORTED: a
// sequence of 2^32 bases or more, or 2^32 pieces or more.
inline cl_status map_piece_first(const uint64_t* seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap, std::vector<uint32_t>& piece_first)
{
	piece_first.assign((size_t)n_seqs + 1, 0);
	if (read_len <= overlap || (n_seqs && !seq_len)) return CL_E_INVALID;
	const uint64_t step = read_len - overlap;
	uint64_t n = 0;
	for (uint32_t s = 0; s < n_seqs; ++s)
	{
		if (seq_len[s] > OV_POS_MAX) return CL_E_UNSUPPORTED;
		n += (seq_len[s] + step - 1) / step;
		if (n > OV_POS_MAX) return CL_E_UNSUPPORTED;
		piece_first[s + 1] = (uint32_t)n;
	}
	return CL_OK;
}

// The lift of one record (t < G.n_pseudo: the caller has checked it, so n_seqs > 0).  Every bound is known before the loop: the search
// halves [lo, hi] within 0 .. n_seqs - 1 and reads piece_first[mid + 1], mid + 1 <= n_seqs, at most 32 times.  Returns the code.
ED_HD inline uint32_t map_lift_one(const MapGeom& G, const cl_overlap& in, cl_overlap& out)
{
	uint32_t lo = 0, hi = G.n_seqs - 1;                                      // the first s with piece_first[s + 1] > t: it exists, piece_first[n_seqs] = n_pseudo > t
	for (uint32_t it = 0; it < 32 && lo < hi; ++it)
	{
		const uint32_t mid = lo + (hi - lo) / 2;
		if (G.piece_first[mid + 1] > in.t) hi = mid; else lo = mid + 1;
	}
	const uint32_t s = lo;
	const uint64_t len = G.seq_len[s], start = (uint64_t)(in.t - G.piece_first[s]) * G.step;      // (start < len < 2^32 by the geometry)
	const uint64_t rest = len > start ? len - start : 0, plen = rest < G.read_len ? rest : G.read_len;
	if (in.tlen != plen) return MAPE_TLEN;
	if (start + in.ts > OV_POS_MAX || start + in.te > OV_POS_MAX) return MAPE_POS;
	if (start + in.te > len) return MAPE_END;
	out = in;
	out.t = s; out.tlen = (uint32_t)len; out.ts = (uint32_t)(start + in.ts); out.te = (uint32_t)(start + in.te); out.flags = in.flags | OV_GENOME;
	return MAPE_NONE;
}

// The host twin of k_map_lift: the records of `in` whose target is a genome piece, lifted and appended to `out` in their order.  false: a
// record is refused — *bad_record / *bad_code name the first — and `out` is unchanged.
inline bool map_lift_host(const MapGeom& G, const cl_overlap* in, uint64_t n, std::vector<cl_overlap>& out, uint64_t* bad_record, uint32_t* bad_code)
{
	std::vector<cl_overlap> B;
	for (uint64_t i = 0; i < n; ++i)
	{
		if (in[i].t >= G.n_pseudo) continue;
		cl_overlap o;
		if (const uint32_t e = map_lift_one(G, in[i], o)) { if (bad_record) *bad_record = i; if (bad_code) *bad_code = e; return false; }
		B.push_back(o);
	}
	out.insert(out.end(), B.begin(), B.end());
	return true;
}
