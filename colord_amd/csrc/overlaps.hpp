// overlaps.hpp — read-to-read overlaps from the edit scripts: every stretch of a read's tuple stream on ONE reference read (a
// VISIT) that holds an aligned column is one record, cl_overlap — where on the read, where on the reference in the reference's forward
// coordinates, how many columns match.  Like the profile (edits.hpp) this is a read against earlier READS, which carry errors of their
// own, and it lists overlaps with reference reads only.  On the device: k_overlap_walk (overlaps.hip).  Here: the record as twelve
// 32-bit words, the codes of a malformed stream (those of edits.hpp) and the host form, a sequential walk over host memory with the
// same checks in the same order and the same answers.
//
// The walk is ed_profile_host's with one more cursor, the read position qpos: ins +1; del cursor +1; match / subst both +1, an aligned
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

// The host form.  References and streams as in ed_profile_host; read r of the batch is read first_read + r of the input; ref_read (or
// null): reference id -> input index of that read, n_ref_read entries — an id at or past it is EDE_REF_ID where the id is met.  false: a
// malformed stream — *bad_read / *bad_code name the first — or a null argument (*bad_code = 0); `out` is unchanged then.  The records of
// the batch are appended to `out`, reads in order, a read's records in visit order.
inline bool ov_walk_host(const uint8_t* ref_codes, const uint64_t* ref_off, uint32_t n_refs, const uint8_t* es, const uint64_t* es_off, uint64_t n_reads, uint64_t first_read,
                         const uint32_t* ref_read, uint32_t n_ref_read, std::vector<cl_overlap>& out, uint64_t* bad_read, uint32_t* bad_code)
{
	if (bad_read) *bad_read = 0;
	if (bad_code) *bad_code = EDE_NONE;
	if ((n_reads && (!es_off || !es)) || (n_refs && (!ref_off || !ref_codes)) || (n_ref_read && !ref_read) || first_read + n_reads > OV_POS_MAX + 1) return false;
	std::vector<cl_overlap> B;
	struct Ref { uint32_t id = 0; uint64_t len = 0; const uint8_t* p = nullptr; bool rev = false; };
	auto ref_base = [](const Ref& c, uint64_t pos) -> uint32_t {
		if (pos >= c.len) return 255;
		const uint32_t b = c.p[c.rev ? c.len - 1 - pos : pos];
		return b > 3 ? 255u : c.rev ? 3u - b : b;
	};
	for (uint64_t r = 0; r < n_reads; ++r)
	{
		auto fail = [&](uint32_t code) { if (bad_read) *bad_read = r; if (bad_code) *bad_code = code; return false; };
		const uint64_t s0 = es_off[r], s1 = es_off[r + 1], n = s1 > s0 ? s1 - s0 : 0;
		const uint8_t* s = es + s0;
		if (!n) return fail(EDE_EMPTY);
		const uint32_t t0 = s[0] >> 4;
		if (t0 == EDT_START_PLAIN || t0 == EDT_START_PLAIN_N)
		{	// a plain read overlaps nothing
			for (uint64_t i = 1; i < n; ++i) { if ((s[i] >> 4) != EDT_PLAIN) return fail(EDE_TYPE); if ((s[i] & 0xf) > 4) return fail(EDE_VALUE); }
			continue;
		}
		if (t0 != EDT_START_ES) return fail(EDE_START);
		if (n < 5) return fail(EDE_TRUNC);
		auto id_at = [&](uint64_t i) { return ((uint32_t)s[i + 1] << 24) | ((uint32_t)s[i + 2] << 16) | ((uint32_t)s[i + 3] << 8) | (uint32_t)s[i + 4]; };
		const uint32_t main_id = id_at(0);
		if (main_id >= n_refs || (ref_read && main_id >= n_ref_read)) return fail(EDE_REF_ID);
		Ref mainc; mainc.id = main_id; mainc.len = ref_off[main_id + 1] - ref_off[main_id]; mainc.p = ref_codes + ref_off[main_id]; mainc.rev = (s[0] & 0xf) != 0;
		Ref cur = mainc;
		uint64_t cursor = 0, main_cursor = 0, qpos = 0; bool is_main = true;
		uint32_t alt_id[ED_MAX_ALT]; bool alt_rev[ED_MAX_ALT]; uint32_t n_alt = 0;
		const size_t first_rec = B.size();
		OvVisit V;
		bool wide = false;                                                      // a reference of 2^32 bases or more gave a record
		auto close = [&]() {
			if (V.has)
			{
				if (cur.len > OV_POS_MAX) wide = true;
				B.push_back(ov_record(V, (uint32_t)(first_read + r), ref_read ? ref_read[cur.id] : cur.id, 0, (uint32_t)cur.len, cur.rev, is_main));
			}
			V = OvVisit();
		};
		auto column = [&](uint64_t q_adv, uint64_t c_adv) {                     // an aligned column (or an anchor's) from qpos / cursor on
			if (!V.has) { V.has = true; V.qs = qpos; V.ts_o = cursor; }
			V.qe = qpos + q_adv; V.te_o = cursor + c_adv;
		};
		uint64_t pos = 5;
		while (pos < n)
		{
			const uint32_t b = s[pos], t = b >> 4, v = b & 0xf;
			if (t > EDT_MAIN_REF) return fail(EDE_TYPE);
			const uint64_t need = t == EDT_ANCHOR || t == EDT_SKIP ? 4 : t == EDT_ALT_ID ? 5 : 1;
			if (pos + need > n) return fail(EDE_TRUNC);
			switch (t)
			{
			case EDT_INS:
				if (v > 3) return fail(EDE_VALUE);
				qpos += 1; break;
			case EDT_DEL: if (ref_base(cur, cursor) > 3) return fail(EDE_GUARD); cursor += 1; break;
			case EDT_MATCH: if (ref_base(cur, cursor) > 3) return fail(EDE_GUARD); column(1, 1); V.matches += 1; qpos += 1; cursor += 1; break;
			case EDT_SUBST:
				if (ref_base(cur, cursor) > 3) return fail(EDE_GUARD);
				if (v > 2) return fail(EDE_VALUE);
				column(1, 1); V.subst += 1; qpos += 1; cursor += 1; break;
			case EDT_ANCHOR: case EDT_SKIP:
			{
				const uint32_t val = (v << 24) | ((uint32_t)s[pos + 1] << 16) | ((uint32_t)s[pos + 2] << 8) | (uint32_t)s[pos + 3];
				if (t == EDT_ANCHOR)
				{
					if (cursor + val > cur.len) return fail(EDE_GUARD);
					if (val) { column(val, val); V.matches += val; V.anchor_bases += val; }
					qpos += val;
				}
				cursor += val; break;
			}
			case EDT_ALT_ID:
			{
				const uint32_t id = id_at(pos);
				if (id >= n_refs || (ref_read && id >= n_ref_read)) return fail(EDE_REF_ID);
				close();
				if (is_main) { main_cursor = cursor; is_main = false; }
				uint32_t k = 0; while (k < n_alt && alt_id[k] != id) ++k;
				if (k == n_alt)
				{	// the orientation of an alternative's first appearance holds
					if (n_alt >= ED_MAX_ALT) return fail(EDE_TOO_MANY_ALT);
					alt_id[k] = id; alt_rev[k] = v != 0; ++n_alt;
				}
				cur.id = id; cur.len = ref_off[id + 1] - ref_off[id]; cur.p = ref_codes + ref_off[id]; cur.rev = alt_rev[k];
				cursor = 0; break;
			}
			default:                                                               // main-ref: closes the visit, and back to the main reference where it was left
				close();
				if (!is_main) { cur = mainc; cursor = main_cursor; is_main = true; }
			}
			pos += need;
		}
		close();
		if (qpos > OV_POS_MAX || wide) return fail(EDE_GUARD);
		for (size_t i = first_rec; i < B.size(); ++i) B[i].qlen = (uint32_t)qpos;
	}
	out.insert(out.end(), B.begin(), B.end());
	return true;
}
