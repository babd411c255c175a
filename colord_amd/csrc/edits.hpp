// edits.hpp — the edit-operation profile: what the compressor did with the bases, counted from the tuple streams of a
// batch and the reference reads they point to.  It is the divergence between a read and the reference READS it was coded against —
// earlier reads, which carry errors of their own — not a per-read error rate (except against the pseudo reads of -G), and it covers
// only what the encoder aligned.  On the device: k_edit_profile (edits.hip).  Here: the layout of cl_edits as an array of 64-bit
// words (what the kernel's cells, the `hipedits` stream and the bindings index), the codes of a malformed stream, and the host form,
// a sequential walk over host memory with the same checks and the same answers.  Every field adds over disjoint sets of reads.
//
// Under a host compiler alone this header needs no HIP (tests/tools/edits_host_test.cpp).
#pragma once
#include <string.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/colord_hip.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ED_HD __host__ __device__
#else
#define ED_HD
#endif

// cl_edits is ED_WORDS counters back to back: the word index of every field
constexpr uint32_t ED_WORDS = sizeof(cl_edits) / 8;
#define ED_AT(field) ((uint32_t)(offsetof(cl_edits, field) / 8))
constexpr uint32_t ED_READS = ED_AT(reads), ED_BASES = ED_AT(bases), ED_KIND_READS = ED_AT(kind_reads), ED_KIND_BASES = ED_AT(kind_bases), ED_KIND_BYTES = ED_AT(kind_bytes),
	ED_MAIN_REV = ED_AT(main_rev), ED_TUPLES = ED_AT(tuples), ED_ANCHOR_BASES = ED_AT(anchor_bases), ED_ANCHOR_LEN = ED_AT(anchor_len_hist), ED_SKIP_ENTRIES = ED_AT(skip_entries),
	ED_SKIP_ENTRY_SUM = ED_AT(skip_entry_sum), ED_SKIP_BASES = ED_AT(skip_bases), ED_SKIP_LEN = ED_AT(skip_len_hist), ED_INS_BASE = ED_AT(ins_base), ED_DEL_BASE = ED_AT(del_base),
	ED_MATCH_BASE = ED_AT(match_base), ED_SUB = ED_AT(sub), ED_INS_RUN = ED_AT(ins_run_hist), ED_DEL_RUN = ED_AT(del_run_hist), ED_IDENTITY = ED_AT(identity_hist),
	ED_IDENTITY_NONE = ED_AT(identity_none), ED_ALT = ED_AT(alt_hist);
static_assert(sizeof(cl_edits) == 312 * 8 && ED_ALT + 65 == ED_WORDS, "cl_edits is 312 counters without padding");
constexpr uint32_t ED_MAX_ALT = 64;
// the tuple types of the stream (es_format.hpp; utils.h:56-273), for the host walk
enum { EDT_INS = 0, EDT_DEL, EDT_MATCH, EDT_SUBST, EDT_ANCHOR, EDT_SKIP, EDT_ALT_ID, EDT_MAIN_REF, EDT_PLAIN, EDT_START_PLAIN, EDT_START_ES, EDT_START_PLAIN_N };
// what a malformed stream ran into
enum { EDE_NONE = 0, EDE_EMPTY, EDE_START, EDE_TYPE, EDE_TRUNC, EDE_REF_ID, EDE_GUARD, EDE_VALUE, EDE_TOO_MANY_ALT, EDE_N };
inline const char* ed_error_text(uint32_t code)
{
	static const char* const T[EDE_N] = { "", "empty stream", "first tuple is no start tuple", "tuple type not allowed inside an edit script", "tuple crosses the end of the stream",
		"reference id outside the reference arena", "position outside the reference read", "base value out of range", "more than 64 alternative references" };
	return code < EDE_N ? T[code] : "?";
}

// bin of an anchor length / a skip value: its bit length (0 -> 0, 1 -> 1, 2..3 -> 2, ..); the values have 28 bits
ED_HD inline uint32_t ed_bit_len(uint32_t v) { uint32_t b = 0; while (v) { ++b; v >>= 1; } return b > 28 ? 28 : b; }
ED_HD inline uint32_t ed_run_bin(uint64_t len) { return len > 16 ? 16u : (uint32_t)len; }
// bin of an edit-script read in identity_hist (m <= d, d > 0)
ED_HD inline uint32_t ed_identity_bin(uint64_t m, uint64_t d) { return (uint32_t)(100 * m / d); }

inline void ed_clear(cl_edits* e) { memset(e, 0, sizeof(*e)); }
inline void ed_add(cl_edits* d, const cl_edits* s)
{
	uint64_t* a = (uint64_t*)d; const uint64_t* b = (const uint64_t*)s;
	for (uint32_t i = 0; i < ED_WORDS; ++i) a[i] += b[i];
}

// The host form.  Reference read i = the codes 0..3 at [ref_off[i], ref_off[i + 1]) of ref_codes; read r = the stream bytes
// [es_off[r], es_off[r + 1]).  false: a malformed stream — *bad_read / *bad_code name the first — or a null argument (*bad_code = 0);
// *acc is unchanged then.  The batch's own profile is complete before anything is added.
inline bool ed_profile_host(const uint8_t* ref_codes, const uint64_t* ref_off, uint32_t n_refs, const uint8_t* es, const uint64_t* es_off, uint64_t n_reads, cl_edits* acc,
                            uint64_t* bad_read, uint32_t* bad_code)
{
	if (bad_read) *bad_read = 0;
	if (bad_code) *bad_code = EDE_NONE;
	if (!acc || (n_reads && (!es_off || !es)) || (n_refs && (!ref_off || !ref_codes))) return false;
	cl_edits B; ed_clear(&B);
	struct Ref { uint32_t id = 0; uint64_t len = 0; const uint8_t* p = nullptr; bool rev = false; };
	// GetRefRead(id, rev)[pos] with the guard 255 (reference_reads.h:142-207)
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
		{
			for (uint64_t i = 1; i < n; ++i) { if ((s[i] >> 4) != EDT_PLAIN) return fail(EDE_TYPE); if ((s[i] & 0xf) > 4) return fail(EDE_VALUE); }
			const uint32_t k = t0 == EDT_START_PLAIN ? 0 : 1;
			B.kind_reads[k] += 1; B.kind_bases[k] += n - 1; B.kind_bytes[k] += n;
			continue;
		}
		if (t0 != EDT_START_ES) return fail(EDE_START);
		if (n < 5) return fail(EDE_TRUNC);
		auto id_at = [&](uint64_t i) { return ((uint32_t)s[i + 1] << 24) | ((uint32_t)s[i + 2] << 16) | ((uint32_t)s[i + 3] << 8) | (uint32_t)s[i + 4]; };
		const uint32_t main_id = id_at(0);
		if (main_id >= n_refs) return fail(EDE_REF_ID);
		Ref mainc; mainc.id = main_id; mainc.len = ref_off[main_id + 1] - ref_off[main_id]; mainc.p = ref_codes + ref_off[main_id]; mainc.rev = (s[0] & 0xf) != 0;
		Ref cur = mainc;
		uint64_t cursor = 0, main_cursor = 0; bool is_main = true;
		uint32_t alt_id[ED_MAX_ALT]; bool alt_rev[ED_MAX_ALT]; uint32_t n_alt = 0;
		uint64_t cnt[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, anchor_bases = 0;
		uint32_t last = EDT_START_ES; uint64_t run = 0;                            // the preceding tuple; the length of the run of ins / del it ends
		auto end_run = [&]() {
			if (!run) return;
			if (last == EDT_INS) B.ins_run_hist[ed_run_bin(run)] += 1; else B.del_run_hist[ed_run_bin(run)] += 1;
			run = 0;
		};
		uint64_t pos = 5;
		while (pos < n)
		{
			const uint32_t b = s[pos], t = b >> 4, v = b & 0xf;
			if (t > EDT_MAIN_REF) return fail(EDE_TYPE);
			const uint64_t need = t == EDT_ANCHOR || t == EDT_SKIP ? 4 : t == EDT_ALT_ID ? 5 : 1;
			if (pos + need > n) return fail(EDE_TRUNC);
			if (t != last) end_run();
			cnt[t] += 1;
			switch (t)
			{
			case EDT_INS:
				if (v > 3) return fail(EDE_VALUE);
				B.ins_base[v] += 1; run += 1; break;
			case EDT_DEL: { const uint32_t rb = ref_base(cur, cursor); if (rb > 3) return fail(EDE_GUARD); B.del_base[rb] += 1; cursor += 1; run += 1; break; }
			case EDT_MATCH: { const uint32_t rb = ref_base(cur, cursor); if (rb > 3) return fail(EDE_GUARD); B.match_base[rb] += 1; cursor += 1; break; }
			case EDT_SUBST:
			{
				const uint32_t rb = ref_base(cur, cursor);
				if (rb > 3) return fail(EDE_GUARD);
				if (v > 2) return fail(EDE_VALUE);
				B.sub[rb][v + (v >= rb ? 1u : 0u)] += 1; cursor += 1; break;
			}
			case EDT_ANCHOR: case EDT_SKIP:
			{
				const uint32_t val = (v << 24) | ((uint32_t)s[pos + 1] << 16) | ((uint32_t)s[pos + 2] << 8) | (uint32_t)s[pos + 3];
				if (t == EDT_ANCHOR)
				{
					if (cursor + val > cur.len) return fail(EDE_GUARD);
					anchor_bases += val; B.anchor_len_hist[ed_bit_len(val)] += 1;
				}
				else if (last == EDT_ALT_ID) { B.skip_entries += 1; B.skip_entry_sum += val; }
				else { B.skip_bases += val; B.skip_len_hist[ed_bit_len(val)] += 1; }
				cursor += val; break;
			}
			case EDT_ALT_ID:
			{
				const uint32_t id = id_at(pos);
				if (id >= n_refs) return fail(EDE_REF_ID);
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
			default:                                                               // main-ref: back to the main reference where it was left
				if (!is_main) { cur = mainc; cursor = main_cursor; is_main = true; }
			}
			last = t; pos += need;
		}
		end_run();
		for (int t = 0; t < 8; ++t) B.tuples[t] += cnt[t];
		const uint64_t m = cnt[EDT_MATCH] + anchor_bases, d = m + cnt[EDT_SUBST] + cnt[EDT_INS] + cnt[EDT_DEL];
		if (d) B.identity_hist[ed_identity_bin(m, d)] += 1; else B.identity_none += 1;
		B.alt_hist[n_alt] += 1; B.main_rev[mainc.rev ? 1 : 0] += 1; B.anchor_bases += anchor_bases;
		B.kind_reads[2] += 1; B.kind_bases[2] += cnt[EDT_INS] + cnt[EDT_MATCH] + cnt[EDT_SUBST] + anchor_bases; B.kind_bytes[2] += n;
	}
	for (int k = 0; k < 3; ++k) { B.reads += B.kind_reads[k]; B.bases += B.kind_bases[k]; }
	ed_add(acc, &B);
	return true;
}
