// cigars.hpp — the base-level CIGAR of every overlap record.  A record is a visit of overlaps.hpp: a stretch of a read's tuple
// stream on ONE reference that holds an aligned column.  Its CIGAR is the sequence of the operations of the visit's tuples in stream order,
//   ins: I 1;  del: D 1;  match: = 1;  subst: X 1;  anchor v: = v;  skip v: D v (an anchor or a skip of 0 gives nothing),
// from the visit's first aligned column to its last, both included — what lies in front of the first (the entry skip behind an alt-id too) and
// behind the last is dropped, the trimming the record's qs / qe / ts / te do —, neighbouring equal operations merged (a zero-length anchor or
// skip between them does not keep them apart).  An operation is one u32, len << 4 | op, with BAM's codes; a merged run of 2^28 bases or more
// does not fit and refuses the read (CGE_RUN).  Operations are in WALK order: the read forward, the reference in the orientation it is taken
// in; a record with OV_REV is reversed by whoever prints it.  On the device: k_cigar_walk (cigars.hip).  Here: what ONE tuple contributes and
// how a run is closed — the functions the kernel and the host twin share, so that the two cannot disagree — and the host twin, a visitor of
// es_walk_host (es_codes.hpp) that owns no check of the walk: a malformed stream gives the read and the code that ov_walk_host gives.
//
// For every record: sum of len(= X I) = qe - qs; sum of len(= X D) = te - ts; sum of len(=) = matches; sum of len(X) = subst; the first and
// the last operation are = or X; no two neighbours are equal; every length is at least 1.
//
// Under a host compiler alone this header needs no HIP (tests/tools/cigars_host_test.cpp).
#pragma once
#include <vector>
#include "overlaps.hpp"

constexpr uint32_t CG_I = 1, CG_D = 2, CG_EQ = 7, CG_X = 8;                 // BAM's codes
constexpr uint32_t CG_OP_BYTES = 4;
constexpr uint64_t CG_LEN_MAX = (1ull << 28) - 1;                           // the longest run a word holds
constexpr uint32_t CGE_RUN = 0x100;                                         // behind the codes of a malformed stream: a run of 2^28 bases or more inside a record

// WHAT ONE TUPLE CONTRIBUTES: the operation of a tuple of type t <= T_SKIP with the 28-bit value val (of an anchor / skip), len = its
// length; len = 0: the tuple gives no operation
ED_HD inline uint32_t cg_tuple(uint32_t t, uint32_t val, uint32_t& len)
{
	switch (t)
	{
	case T_INS: len = 1; return CG_I;
	case T_DEL: len = 1; return CG_D;
	case T_MATCH: len = 1; return CG_EQ;
	case T_SUBST: len = 1; return CG_X;
	case T_ANCHOR: len = val; return CG_EQ;
	case T_SKIP: len = val; return CG_D;
	}
	len = 0; return 0;
}
// an operation that is an aligned column (or a row of them)
ED_HD inline bool cg_aligned(uint32_t op) { return op == CG_EQ || op == CG_X; }
// HOW A RUN IS CLOSED: the word of a merged run of len >= 1 bases; false: the run does not fit
ED_HD inline bool cg_word(uint32_t op, uint64_t len, uint32_t& w)
{
	if (len > CG_LEN_MAX) return false;
	w = ((uint32_t)len << 4) | op;
	return true;
}
ED_HD inline uint32_t cg_op(uint32_t w) { return w & 0xf; }
ED_HD inline uint32_t cg_len(uint32_t w) { return w >> 4; }
inline char cg_char(uint32_t op) { return op == CG_I ? 'I' : op == CG_D ? 'D' : op == CG_EQ ? '=' : op == CG_X ? 'X' : '?'; }
// the codes of cl_cigars_host's bad_code: those of the walk, and CGE_RUN
inline const char* cg_error_text(uint32_t code) { return code == CGE_RUN ? "a CIGAR operation of 2^28 bases or more" : ed_error_text(code); }

// the relations above of one record's operations against its record; 0, or the number of the first that is broken (1 .. 7 in the order above)
inline uint32_t cg_check(const cl_overlap& o, const uint32_t* ops, uint64_t n)
{
	uint64_t q = 0, t = 0, eq = 0, x = 0;
	if (!n || !cg_aligned(cg_op(ops[0])) || !cg_aligned(cg_op(ops[n - 1]))) return 5;
	for (uint64_t i = 0; i < n; ++i)
	{
		const uint32_t op = cg_op(ops[i]), len = cg_len(ops[i]);
		if (op != CG_I && op != CG_D && op != CG_EQ && op != CG_X) return 5;
		if (i && op == cg_op(ops[i - 1])) return 6;
		if (!len) return 7;
		if (op != CG_D) q += len;
		if (op != CG_I) t += len;
		if (op == CG_EQ) eq += len;
		if (op == CG_X) x += len;
	}
	if (o.qe < o.qs || q != (uint64_t)(o.qe - o.qs)) return 1;
	if (o.te < o.ts || t != (uint64_t)(o.te - o.ts)) return 2;
	if (eq != o.matches) return 3;
	if (x != o.subst) return 4;
	return 0;
}

// The host twin: es_walk_host with the visitor that keeps every visit's runs.  id_limit: a visit on a reference id at or past it gets a count
// of 0 and no operation (0: every reference).  rec_ops: a count per record, in the order of ov_walk_host's records; ops: the operations of
// the records one behind the other.
struct CgHostVisitor {
	uint32_t id_limit;
	std::vector<uint32_t> rec_ops, ops;
	struct Run { uint32_t op; uint64_t len; };
	std::vector<Run> runs;                                                     // of the open visit, from its first aligned column on, merged
	size_t keep = 0;                                                           // ... and how many of them there were at its last aligned column
	bool too_long = false;                                                     // of the read: a kept run does not fit its word
	uint64_t qpos = 0;                                                         // ... and its position, for the overlaps' refusal of one past 2^32 - 1
	void close(const EsHostWalk& W)
	{
		if (!runs.empty())
		{
			const bool counted = W.cur.id < id_limit;
			for (size_t i = 0; counted && i < keep; ++i)
			{
				uint32_t w = 0;
				if (!cg_word(runs[i].op, runs[i].len, w)) too_long = true;
				ops.push_back(w);
			}
			rec_ops.push_back(counted ? (uint32_t)keep : 0u);
		}
		runs.clear(); keep = 0;
	}
	void plain(uint32_t, uint64_t) {}
	void begin(const EsHostWalk&) { runs.clear(); keep = 0; too_long = false; qpos = 0; }
	void tuple(const EsHostWalk& W, uint32_t t, uint32_t, uint32_t val, uint32_t)
	{
		if (t > T_SKIP) { close(W); return; }                                  // alt-id, main-ref: every one closes the visit
		uint32_t len = 0; const uint32_t op = cg_tuple(t, val, len);
		if (op != CG_D) qpos += len;
		if (!len || (runs.empty() && !cg_aligned(op))) return;                // nothing, or in front of the first aligned column
		if (!runs.empty() && runs.back().op == op) runs.back().len += len; else runs.push_back(Run{ op, len });
		if (cg_aligned(op)) keep = runs.size();
	}
	uint32_t end(const EsHostWalk& W, uint64_t n)
	{
		close(W);
		if (qpos > OV_POS_MAX || n > OV_POS_MAX) return EDE_GUARD;            // as the overlaps; and a record's count is 32 bits (a tuple has a byte at the least)
		return too_long ? CGE_RUN : (uint32_t)EDE_NONE;
	}
};
// The counts and operations of a batch appended to rec_ops / ops.  false: a malformed stream or a run that does not fit — *bad_read /
// *bad_code name the first — or a null argument (*bad_code = 0); the outputs are unchanged then.
inline bool cg_walk_host(const uint8_t* ref_codes, const uint64_t* ref_off, uint32_t n_refs, const uint8_t* es, const uint64_t* es_off, uint64_t n_reads, uint32_t id_limit,
                         std::vector<uint32_t>& rec_ops, std::vector<uint32_t>& ops, uint64_t* bad_read, uint32_t* bad_code)
{
	CgHostVisitor vis{ id_limit ? id_limit : 0xffffffffu };
	if (!es_walk_host(ref_codes, ref_off, n_refs, n_refs, es, es_off, n_reads, true, vis, bad_read, bad_code)) return false;
	rec_ops.insert(rec_ops.end(), vis.rec_ops.begin(), vis.rec_ops.end());
	ops.insert(ops.end(), vis.ops.begin(), vis.ops.end());
	return true;
}
