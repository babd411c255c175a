// edits.hpp — the edit-operation profile: what the compressor did with the bases, counted from the tuple streams of a
// batch and the reference reads they point to.  It is the divergence between a read and the reference READS it was coded against —
// earlier reads, which carry errors of their own — not a per-read error rate (except against the pseudo reads of -G), and it covers
// only what the encoder aligned.  On the device: k_edit_profile (edits.hip).  Here: the layout of cl_edits as an array of 64-bit
// words (what the kernel's cells, the `hipedits` stream and the bindings index) and the host form, the visitor of es_walk_host
// (es_codes.hpp: the tuple types, the codes of a malformed stream, the walk and its checks) that counts.  Every field adds over
// disjoint sets of reads.
//
// Under a host compiler alone this header needs no HIP (tests/tools/edits_host_test.cpp).
#pragma once
#include <string.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/colord_hip.h"
#include "es_codes.hpp"
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


// The host form: es_walk_host (es_codes.hpp) with the visitor that counts.  References and streams as there.  false: a malformed stream —
// *bad_read / *bad_code name the first — or a null argument (*bad_code = 0); *acc is unchanged then.  The batch's own profile is complete
// before anything is added.
struct EdProfileVisitor {
	cl_edits B;
	uint64_t cnt[8], anchor_bases, run;                                         // of the read: tuples by type; the length of the run of ins / del the preceding tuple ends
	void end_run(uint32_t last)
	{
		if (!run) return;
		if (last == T_INS) B.ins_run_hist[ed_run_bin(run)] += 1; else B.del_run_hist[ed_run_bin(run)] += 1;
		run = 0;
	}
	void plain(uint32_t t0, uint64_t n) { const uint32_t k = t0 == T_START_PLAIN ? 0 : 1; B.kind_reads[k] += 1; B.kind_bases[k] += n - 1; B.kind_bytes[k] += n; }
	void begin(const EsHostWalk&) { for (uint64_t& c : cnt) c = 0; anchor_bases = run = 0; }
	void tuple(const EsHostWalk& W, uint32_t t, uint32_t v, uint32_t val, uint32_t rb)
	{
		if (t != W.last) end_run(W.last);
		cnt[t] += 1;
		switch (t)
		{
		case T_INS: B.ins_base[v] += 1; run += 1; break;
		case T_DEL: B.del_base[rb] += 1; run += 1; break;
		case T_MATCH: B.match_base[rb] += 1; break;
		case T_SUBST: B.sub[rb][v + (v >= rb ? 1u : 0u)] += 1; break;
		case T_ANCHOR: anchor_bases += val; B.anchor_len_hist[ed_bit_len(val)] += 1; break;
		case T_SKIP:
			if (W.last == T_ALT_ID) { B.skip_entries += 1; B.skip_entry_sum += val; }
			else { B.skip_bases += val; B.skip_len_hist[ed_bit_len(val)] += 1; }
		}
	}
	uint32_t end(const EsHostWalk& W, uint64_t n)
	{
		end_run(W.last);
		for (int t = 0; t < 8; ++t) B.tuples[t] += cnt[t];
		const uint64_t m = cnt[T_MATCH] + anchor_bases, d = m + cnt[T_SUBST] + cnt[T_INS] + cnt[T_DEL];
		if (d) B.identity_hist[ed_identity_bin(m, d)] += 1; else B.identity_none += 1;
		B.alt_hist[W.n_alt] += 1; B.main_rev[W.mainc.rev ? 1 : 0] += 1; B.anchor_bases += anchor_bases;
		B.kind_reads[2] += 1; B.kind_bases[2] += cnt[T_INS] + cnt[T_MATCH] + cnt[T_SUBST] + anchor_bases; B.kind_bytes[2] += n;
		return EDE_NONE;
	}
};
inline bool ed_profile_host(const uint8_t* ref_codes, const uint64_t* ref_off, uint32_t n_refs, const uint8_t* es, const uint64_t* es_off, uint64_t n_reads, cl_edits* acc,
                            uint64_t* bad_read, uint32_t* bad_code)
{
	EdProfileVisitor vis; ed_clear(&vis.B);
	if (!es_walk_host(ref_codes, ref_off, n_refs, n_refs, es, es_off, n_reads, acc != nullptr, vis, bad_read, bad_code)) return false;
	for (int k = 0; k < 3; ++k) { vis.B.reads += vis.B.kind_reads[k]; vis.B.bases += vis.B.kind_bases[k]; }
	ed_add(acc, &vis.B);
	return true;
}
