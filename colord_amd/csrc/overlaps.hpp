// overlaps.hpp — read-to-read overlaps from the edit scripts: every stretch of a read's tuple stream on ONE reference read (a
// VISIT) that holds an aligned column is one record, cl_overlap — where on the read, where on the reference in the reference's forward
// coordinates, how many columns match.  Like the profile (edits.hpp) this is a read against earlier READS, which carry errors of their
// own, and it lists overlaps with reference reads only.  On the device: k_overlap_walk (overlaps.hip).  Here: the record as twelve
// 32-bit words and the host form, the visitor of es_walk_host (es_codes.hpp: the tuple types, the codes of a malformed stream, the walk
// and its checks) that keeps the visits.
//
// The visitor adds one more cursor to the walk's, the read position qpos: ins +1; del cursor +1; match / subst both +1, an aligned
// column; anchor v both +v, aligned iff v > 0; skip v cursor +v (the entry skip behind an alt-id too).  A visit opens behind start-es and
// behind every alt-id / main-ref tuple; every alt-id and main-ref closes the open one (a main-ref met on the main reference too), and so
// does the stream's end.  qs / ts_o: qpos / cursor in front of the visit's first aligned column, qe / te_o: behind its last.
//
// Under a host compiler alone this header needs no HIP (tests/tools/overlaps_host_test.cpp).
#pragma once
#include <vector>
#include "edits.hpp"

constexpr uint32_t OV_WORDS = 12;
static_assert(sizeof(cl_overlap) == OV_WORDS * 4, "cl_overlap is twelve 32-bit words without padding");
constexpr uint32_t OV_REV = 1, OV_MAIN = 2;                                 // flags
constexpr uint64_t OV_POS_MAX = 0xffffffffULL;                              // a position past it makes the stream malformed (EDE_GUARD)

// what a visit has gathered; positions as the walk has them (the target's in the orientation the reference is taken in)
struct OvVisit { bool has = false; uint64_t qs = 0, qe = 0, ts_o = 0, te_o = 0, matches = 0, subst = 0, anchor_bases = 0; };
// the record of a visit that holds an aligned column (te_o <= tlen: every aligned column was checked against the reference's end)
ED_HD inline cl_overlap ov_record(const OvVisit& v, uint32_t q, uint32_t t, uint32_t qlen, uint32_t tlen, bool rev, bool is_main)
{
	cl_overlap o;
	o.q = q; o.t = t; o.qlen = qlen; o.tlen = tlen; o.qs = (uint32_t)v.qs; o.qe = (uint32_t)v.qe;
	o.ts = rev ? tlen - (uint32_t)v.te_o : (uint32_t)v.ts_o; o.te = rev ? tlen - (uint32_t)v.ts_o : (uint32_t)v.te_o;
	o.matches = (uint32_t)v.matches; o.subst = (uint32_t)v.subst; o.anchor_bases = (uint32_t)v.anchor_bases;
	o.flags = (rev ? OV_REV : 0u) | (is_main ? OV_MAIN : 0u);
	return o;
}
// the alignment block length of a record, which is not stored: aligned columns + insertions + deletions between qs / qe and ts / te
inline uint64_t ov_block(const cl_overlap& o) { return (uint64_t)(o.qe - o.qs) + (o.te - o.ts) - o.matches - o.subst; }

// The host form: es_walk_host (es_codes.hpp) with the visitor that keeps the visits.  References and streams as there; read r of the batch is
// read first_read + r of the input; ref_read (or null): reference id -> input index of that read, n_ref_read entries — an id at or past it is
// EDE_REF_ID where the id is met.  false: a malformed stream — *bad_read / *bad_code name the first — or a null argument (*bad_code = 0);
// `out` is unchanged then.  The records of the batch are appended to `out`, reads in order, a read's records in visit order.
struct OvHostVisitor {
	uint64_t first_read; const uint32_t* ref_read;
	std::vector<cl_overlap> B;
	size_t first_rec = 0; uint64_t qpos = 0; OvVisit V;                         // of the read: its first record, the read position, the open visit
	bool wide = false;                                                          // a reference of 2^32 bases or more gave a record
	void close(const EsHostWalk& W)
	{
		if (V.has)
		{
			if (W.cur.len > OV_POS_MAX) wide = true;
			B.push_back(ov_record(V, (uint32_t)(first_read + W.read), ref_read ? ref_read[W.cur.id] : W.cur.id, 0, (uint32_t)W.cur.len, W.cur.rev, W.is_main));
		}
		V = OvVisit();
	}
	void column(const EsHostWalk& W, uint64_t adv)                              // an aligned column (or an anchor's) from qpos / cursor on
	{
		if (!V.has) { V.has = true; V.qs = qpos; V.ts_o = W.cursor; }
		V.qe = qpos + adv; V.te_o = W.cursor + adv;
	}
	void plain(uint32_t, uint64_t) {}                                           // a plain read overlaps nothing
	void begin(const EsHostWalk&) { first_rec = B.size(); qpos = 0; V = OvVisit(); wide = false; }
	void tuple(const EsHostWalk& W, uint32_t t, uint32_t, uint32_t val, uint32_t)
	{
		switch (t)
		{
		case T_INS: qpos += 1; break;
		case T_MATCH: column(W, 1); V.matches += 1; qpos += 1; break;
		case T_SUBST: column(W, 1); V.subst += 1; qpos += 1; break;
		case T_ANCHOR:
			if (val) { column(W, val); V.matches += val; V.anchor_bases += val; }
			qpos += val; break;
		case T_ALT_ID: case T_MAIN_REF: close(W);                              // every one closes the visit (a main-ref met on the main reference too)
		}
	}
	uint32_t end(const EsHostWalk& W, uint64_t)
	{
		close(W);
		if (qpos > OV_POS_MAX || wide) return EDE_GUARD;
		for (size_t i = first_rec; i < B.size(); ++i) B[i].qlen = (uint32_t)qpos;
		return EDE_NONE;
	}
};
inline bool ov_walk_host(const uint8_t* ref_codes, const uint64_t* ref_off, uint32_t n_refs, const uint8_t* es, const uint64_t* es_off, uint64_t n_reads, uint64_t first_read,
                         const uint32_t* ref_read, uint32_t n_ref_read, std::vector<cl_overlap>& out, uint64_t* bad_read, uint32_t* bad_code)
{
	OvHostVisitor vis{ first_read, ref_read };
	const bool args_ok = !(n_ref_read && !ref_read) && first_read + n_reads <= OV_POS_MAX + 1;
	if (!es_walk_host(ref_codes, ref_off, n_refs, ref_read ? n_ref_read : n_refs, es, es_off, n_reads, args_ok, vis, bad_read, bad_code)) return false;
	out.insert(out.end(), vis.B.begin(), vis.B.end());
	return true;
}
