// es_codes.hpp — the tuple-stream byte format (es_t, utils.h:56-273) as ONE decision for everything that walks it: the tuple types, the
// codes of a malformed stream with their texts, and the host walk, es_walk_host.  The device's wave-level walk is es_wave.hpp; both fire
// the same checks in the same order.
//   type in the high nibble of the first byte;  1 byte: ins, del, match, subst, main-ref, plain, start-plain, start-plain-with-Ns;
//   4 bytes: anchor, skip (28-bit big-endian value);  5 bytes: alt-id, start-es (low nibble = orientation, 32-bit big-endian id)
//
// This header needs no HIP: it builds under a host compiler alone (tests/tools/edits_host_test.cpp, overlaps_host_test.cpp).
#pragma once
#include <stdint.h>

enum { T_INS = 0, T_DEL, T_MATCH, T_SUBST, T_ANCHOR, T_SKIP, T_ALT_ID, T_MAIN_REF, T_PLAIN, T_START_PLAIN, T_START_ES, T_START_PLAIN_N, T_NONE };
constexpr uint32_t ED_MAX_ALT = 64;                                         // alternative references of one read
// what a malformed stream ran into; behind EDE_TOO_MANY_ALT what only the expander (expand.hip) can meet
enum { EDE_NONE = 0, EDE_EMPTY, EDE_START, EDE_TYPE, EDE_TRUNC, EDE_REF_ID, EDE_GUARD, EDE_VALUE, EDE_TOO_MANY_ALT, EDE_OUT_RANGE, EDE_TOO_LONG, EDE_NTUP, EDE_N };
inline const char* es_error_text(uint32_t code)
{
	static const char* const T[EDE_N] = { "", "empty stream", "first tuple is no start tuple", "tuple type not allowed inside an edit script", "tuple crosses the end of the stream",
		"reference id outside the reference arena", "position outside the reference read", "base value out of range", "more than 64 alternative references",
		"more bases than the length pass measured", "more than 2^32 - 1 bases", "tuple count differs from the one given" };
	return code < EDE_N ? T[code] : "?";
}
// the codes of the profile and the overlaps, which expand nothing
inline const char* ed_error_text(uint32_t code) { return code <= EDE_TOO_MANY_ALT ? es_error_text(code) : "?"; }

// a reference read of the host walk: the codes 0..3 at p
struct EsHostRef { uint32_t id = 0; uint64_t len = 0; const uint8_t* p = nullptr; bool rev = false; };
// GetRefRead(id, rev)[pos] with the guard 255 (reference_reads.h:142-207)
inline uint32_t ref_base(const EsHostRef& c, uint64_t pos)
{
	if (pos >= c.len) return 255;
	const uint32_t b = c.p[c.rev ? c.len - 1 - pos : pos];
	return b > 3 ? 255u : c.rev ? 3u - b : b;
}
// where the host walk stands in front of a tuple
struct EsHostWalk { uint64_t read = 0; EsHostRef mainc, cur; uint64_t cursor = 0, main_cursor = 0; bool is_main = true; uint32_t n_alt = 0, last = T_START_ES; };

// The host walk: a sequential walk over host memory.  Reference read i = the codes 0..3 at [ref_off[i], ref_off[i + 1]) of ref_codes, ids
// below id_limit <= n_refs; read r = the stream bytes [es_off[r], es_off[r + 1]).  false: a malformed stream — *bad_read / *bad_code name the
// first — or a null argument or !args_ok (*bad_code = 0).  It owns every check and the reference state; the visitor sees only what passed:
//   vis.plain(t0, n)               a plain read of n stream bytes, checked
//   vis.begin(W)                   an edit-script read, W behind its start tuple
//   vis.tuple(W, t, v, val, rb)    a tuple in front of which the walk stands at W (W.last = the tuple before): v = its low nibble, val = the
//                                  28-bit value of an anchor / skip, rb = the reference base of a del / match / subst; the cursor advance
//                                  and the change of reference follow the call
//   vis.end(W, n)                  the stream's end; an error code of its own, or EDE_NONE
// The order of the checks: empty; start tuple (plain kinds, else START, TRUNC, REF_ID); per tuple TYPE, TRUNC, then ins VALUE; del / match
// GUARD; subst GUARD, VALUE; anchor GUARD; alt-id REF_ID, TOO_MANY_ALT.
template<class V>
inline bool es_walk_host(const uint8_t* ref_codes, const uint64_t* ref_off, uint32_t n_refs, uint32_t id_limit, const uint8_t* es, const uint64_t* es_off, uint64_t n_reads, bool args_ok,
                         V& vis, uint64_t* bad_read, uint32_t* bad_code)
{
	if (bad_read) *bad_read = 0;
	if (bad_code) *bad_code = EDE_NONE;
	if (!args_ok || (n_reads && (!es_off || !es)) || (n_refs && (!ref_off || !ref_codes))) return false;
	if (id_limit > n_refs) id_limit = n_refs;
	for (uint64_t r = 0; r < n_reads; ++r)
	{
		auto fail = [&](uint32_t code) { if (bad_read) *bad_read = r; if (bad_code) *bad_code = code; return false; };
		const uint64_t s0 = es_off[r], s1 = es_off[r + 1], n = s1 > s0 ? s1 - s0 : 0;
		const uint8_t* s = es + s0;
		if (!n) return fail(EDE_EMPTY);
		const uint32_t t0 = s[0] >> 4;
		if (t0 == T_START_PLAIN || t0 == T_START_PLAIN_N)
		{
			for (uint64_t i = 1; i < n; ++i) { if ((s[i] >> 4) != T_PLAIN) return fail(EDE_TYPE); if ((s[i] & 0xf) > 4) return fail(EDE_VALUE); }
			vis.plain(t0, n);
			continue;
		}
		if (t0 != T_START_ES) return fail(EDE_START);
		if (n < 5) return fail(EDE_TRUNC);
		auto id_at = [&](uint64_t i) { return ((uint32_t)s[i + 1] << 24) | ((uint32_t)s[i + 2] << 16) | ((uint32_t)s[i + 3] << 8) | (uint32_t)s[i + 4]; };
		auto ref_of = [&](uint32_t id, bool rev) { EsHostRef c; c.id = id; c.len = ref_off[id + 1] - ref_off[id]; c.p = ref_codes + ref_off[id]; c.rev = rev; return c; };
		const uint32_t main_id = id_at(0);
		if (main_id >= id_limit) return fail(EDE_REF_ID);
		EsHostWalk W; W.read = r; W.mainc = W.cur = ref_of(main_id, (s[0] & 0xf) != 0);
		uint32_t alt_id[ED_MAX_ALT]; bool alt_rev[ED_MAX_ALT];
		vis.begin(W);
		uint64_t pos = 5;
		while (pos < n)
		{
			const uint32_t b = s[pos], t = b >> 4, v = b & 0xf;
			if (t > T_MAIN_REF) return fail(EDE_TYPE);
			const uint64_t need = t == T_ANCHOR || t == T_SKIP ? 4 : t == T_ALT_ID ? 5 : 1;
			if (pos + need > n) return fail(EDE_TRUNC);
			uint32_t val = 0, rb = 255;
			if (t == T_INS) { if (v > 3) return fail(EDE_VALUE); }
			else if (t <= T_SUBST)
			{
				rb = ref_base(W.cur, W.cursor);
				if (rb > 3) return fail(EDE_GUARD);
				if (t == T_SUBST && v > 2) return fail(EDE_VALUE);
				val = 1;
			}
			else if (t <= T_SKIP)
			{
				val = (v << 24) | ((uint32_t)s[pos + 1] << 16) | ((uint32_t)s[pos + 2] << 8) | (uint32_t)s[pos + 3];
				if (t == T_ANCHOR && W.cursor + val > W.cur.len) return fail(EDE_GUARD);
			}
			else if (t == T_ALT_ID)
			{
				const uint32_t id = id_at(pos);
				if (id >= id_limit) return fail(EDE_REF_ID);
				uint32_t k = 0; while (k < W.n_alt && alt_id[k] != id) ++k;
				if (k == W.n_alt && k >= ED_MAX_ALT) return fail(EDE_TOO_MANY_ALT);
				vis.tuple(W, t, v, 0u, 255u);
				if (k == W.n_alt) { alt_id[k] = id; alt_rev[k] = v != 0; ++W.n_alt; }      // the orientation of an alternative's first appearance holds
				if (W.is_main) { W.main_cursor = W.cursor; W.is_main = false; }
				W.cur = ref_of(id, alt_rev[k]); W.cursor = 0;
			}
			else
			{	// main-ref: back to the main reference where it was left
				vis.tuple(W, t, v, 0u, 255u);
				if (!W.is_main) { W.cur = W.mainc; W.cursor = W.main_cursor; W.is_main = true; }
			}
			if (t <= T_SKIP) { vis.tuple(W, t, v, val, rb); W.cursor += val; }
			W.last = t; pos += need;
		}
		const uint32_t code = vis.end(W, n);
		if (code) return fail(code);
	}
	return true;
}
