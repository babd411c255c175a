// edits_stream.hpp — the `hipedits` stream of an archive: the edit-operation profile of the tuple streams, counted on the
// device right after the edit scripts were made (`colord_hip compress-* --edit-profile`), printed by `colord_hip info [--edit-profile
// [--json]]` without decoding anything.  One part, little-endian, of a fixed size:
//   u32 version = 1, u32 flags = 0, then every field of cl_edits in its order as u64 (312 of them)
// Shares, rates and means are made when printing and never stored.  The reference's decompressor finds its streams by name and never
// sees this one; `decompress` and `check` do not recompute it (that would put counters into the decoder's loop).
// WHAT IT IS: the divergence between a read and the reference READS it was coded against, which carry errors of their own — not a
// per-read error rate, except against the pseudo reads of -G — and only of what the encoder aligned.
#pragma once
#include "archive.hpp"
#include "../edits.hpp"
#include <memory>

struct EditsSet {
	std::unique_ptr<cl_edits> e{ new cl_edits };
	EditsSet() { ed_clear(e.get()); }
	static constexpr size_t BYTES = 8 + 8 * (size_t)ED_WORDS;
	std::vector<uint8_t> pack() const
	{
		std::vector<uint8_t> v;
		auto le = [&](uint64_t x, int n) { for (int i = 0; i < n; ++i) v.push_back((uint8_t)(x >> (8 * i))); };
		le(1, 4); le(0, 4);
		const uint64_t* w = (const uint64_t*)e.get();
		for (uint32_t i = 0; i < ED_WORDS; ++i) le(w[i], 8);
		return v;
	}
	// false: another version, other flags, another size
	bool unpack(const std::vector<uint8_t>& v)
	{
		ed_clear(e.get());
		if (v.size() != BYTES) return false;
		auto le = [&](size_t at, int n) { uint64_t x = 0; for (int i = 0; i < n; ++i) x |= (uint64_t)v[at + i] << (8 * i); return x; };
		if (le(0, 4) != 1 || le(4, 4) != 0) return false;
		uint64_t* w = (uint64_t*)e.get();
		for (uint32_t i = 0; i < ED_WORDS; ++i) w[i] = le(8 + 8 * (size_t)i, 8);
		return true;
	}
};

// the stored profile of an archive: 0 none, 1 read, -1 a `hipedits` stream this build cannot read
inline int read_hipedits(const std::string& path, EditsSet& out)
{
	ArchiveReader ar;
	if (!ar.open(path)) return 0;
	const int s = ar.id("hipedits");
	std::vector<uint8_t> b; uint64_t meta = 0; int r = 0;
	if (s >= 0) r = ar.part(s, 0, b, meta) && out.unpack(b) ? 1 : -1;
	ar.close();
	return r;
}

// what is made of the counters when printing
struct EditsDerived {
	double kind_read_share[3] = { 0, 0, 0 }, kind_base_share[3] = { 0, 0, 0 };
	double anchor_base_share = 0;                      // of the bases of edit-script reads
	uint64_t aligned = 0;                              // match + anchor bases + subst + ins + del
	double sub_rate = 0, ins_rate = 0, del_rate = 0;   // per aligned base
	uint64_t transitions = 0, transversions = 0;
	double ins_run_mean = 0, del_run_mean = 0, ins_in_runs2 = 0, del_in_runs2 = 0;   // mean run length; share of the ins (del) tuples that lie in runs of 2 or more
	int identity_median = -1;                          // bin of the median read, -1 without one
	double alts_per_read = 0;
};
inline EditsDerived edits_derived(const cl_edits& e)
{
	EditsDerived D;
	auto ratio = [](uint64_t a, uint64_t b) { return b ? (double)a / (double)b : 0.0; };
	for (int k = 0; k < 3; ++k) { D.kind_read_share[k] = ratio(e.kind_reads[k], e.reads); D.kind_base_share[k] = ratio(e.kind_bases[k], e.bases); }
	D.anchor_base_share = ratio(e.anchor_bases, e.kind_bases[2]);
	D.aligned = e.tuples[2] + e.anchor_bases + e.tuples[3] + e.tuples[0] + e.tuples[1];
	D.sub_rate = ratio(e.tuples[3], D.aligned); D.ins_rate = ratio(e.tuples[0], D.aligned); D.del_rate = ratio(e.tuples[1], D.aligned);
	for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) if (i != j) { if ((i ^ j) == 2) D.transitions += e.sub[i][j]; else D.transversions += e.sub[i][j]; }   // A<->G, C<->T
	uint64_t iruns = 0, druns = 0;
	for (int i = 0; i < 17; ++i) { iruns += e.ins_run_hist[i]; druns += e.del_run_hist[i]; }
	D.ins_run_mean = ratio(e.tuples[0], iruns); D.del_run_mean = ratio(e.tuples[1], druns);
	D.ins_in_runs2 = ratio(e.tuples[0] - (e.tuples[0] >= e.ins_run_hist[1] ? e.ins_run_hist[1] : e.tuples[0]), e.tuples[0]);
	D.del_in_runs2 = ratio(e.tuples[1] - (e.tuples[1] >= e.del_run_hist[1] ? e.del_run_hist[1] : e.tuples[1]), e.tuples[1]);
	uint64_t with_id = 0; for (int i = 0; i <= 100; ++i) with_id += e.identity_hist[i];
	if (with_id) { uint64_t run = 0; for (int i = 0; i <= 100; ++i) { run += e.identity_hist[i]; if (2 * run >= with_id) { D.identity_median = i; break; } } }
	uint64_t alts = 0; for (int i = 0; i <= 64; ++i) alts += (uint64_t)i * e.alt_hist[i];
	D.alts_per_read = ratio(alts, e.kind_reads[2]);
	return D;
}
inline const char* const EDITS_NOTE = "divergence between each read and the reference READS it was coded against (both carry errors): not a per-read error rate, except against -G pseudo reads; only what the encoder aligned";
inline void print_edits(FILE* f, const EditsSet& S)
{
	const cl_edits& e = *S.e; const EditsDerived D = edits_derived(e);
	auto u = [](uint64_t x) { return (unsigned long long)x; };
	static const char* const kind[3] = { "plain", "plain with Ns", "edit script" };
	static const char* const type[8] = { "ins", "del", "match", "subst", "anchor", "skip", "alt-id", "main-ref" };
	fprintf(f, "edit profile: %s\n", EDITS_NOTE);
	fprintf(f, "reads: %llu\nbases: %llu\n", u(e.reads), u(e.bases));
	for (int k = 0; k < 3; ++k) fprintf(f, "coded as %s: %llu reads (%.4f), %llu bases (%.4f), %llu stream bytes\n", kind[k], u(e.kind_reads[k]), D.kind_read_share[k], u(e.kind_bases[k]), D.kind_base_share[k], u(e.kind_bytes[k]));
	fprintf(f, "main reference: %llu forward, %llu reversed\n", u(e.main_rev[0]), u(e.main_rev[1]));
	fprintf(f, "tuples:"); for (int t = 0; t < 8; ++t) fprintf(f, " %s %llu%s", type[t], u(e.tuples[t]), t < 7 ? "," : "\n");
	fprintf(f, "anchors: %llu bases, %.4f of the bases of edit-script reads\n", u(e.anchor_bases), D.anchor_base_share);
	fprintf(f, "aligned bases: %llu; per aligned base: subst %.6f, ins %.6f, del %.6f\n", u(D.aligned), D.sub_rate, D.ins_rate, D.del_rate);
	fprintf(f, "transitions : transversions = %llu : %llu\n", u(D.transitions), u(D.transversions));
	fprintf(f, "substitutions (reference base -> read base: A C G T):\n");
	for (int i = 0; i < 4; ++i) fprintf(f, "  %c  %llu %llu %llu %llu\n", "ACGT"[i], u(e.sub[i][0]), u(e.sub[i][1]), u(e.sub[i][2]), u(e.sub[i][3]));
	fprintf(f, "inserted bases: A %llu, C %llu, G %llu, T %llu\n", u(e.ins_base[0]), u(e.ins_base[1]), u(e.ins_base[2]), u(e.ins_base[3]));
	fprintf(f, "deleted reference bases: A %llu, C %llu, G %llu, T %llu\n", u(e.del_base[0]), u(e.del_base[1]), u(e.del_base[2]), u(e.del_base[3]));
	fprintf(f, "matched reference bases: A %llu, C %llu, G %llu, T %llu\n", u(e.match_base[0]), u(e.match_base[1]), u(e.match_base[2]), u(e.match_base[3]));
	fprintf(f, "insertion runs: mean length %.3f, %.4f of the insertions in runs of 2 or more\n", D.ins_run_mean, D.ins_in_runs2);
	fprintf(f, "deletion runs: mean length %.3f, %.4f of the deletions in runs of 2 or more\n", D.del_run_mean, D.del_in_runs2);
	fprintf(f, "runs by length (length: insertion runs, deletion runs; 16 = 16 and more):\n");
	for (int i = 1; i < 17; ++i) if (e.ins_run_hist[i] || e.del_run_hist[i]) fprintf(f, "  %2d  %llu  %llu\n", i, u(e.ins_run_hist[i]), u(e.del_run_hist[i]));
	fprintf(f, "anchors and skips by bit length of the length (bin: anchors, skips):\n");
	for (int i = 0; i < 29; ++i) if (e.anchor_len_hist[i] || e.skip_len_hist[i]) fprintf(f, "  %2d  %llu  %llu\n", i, u(e.anchor_len_hist[i]), u(e.skip_len_hist[i]));
	fprintf(f, "skipped reference bases: %llu; entries into alternatives: %llu (sum of the entry positions %llu)\n", u(e.skip_bases), u(e.skip_entries), u(e.skip_entry_sum));
	if (D.identity_median >= 0) fprintf(f, "identity per edit-script read (floor of 100 x (match + anchor bases) / aligned bases: reads); median bin %d; %llu reads without an aligned base:\n", D.identity_median, u(e.identity_none));
	else fprintf(f, "identity per edit-script read: none with an aligned base (%llu without)\n", u(e.identity_none));
	for (int i = 0; i <= 100; ++i) if (e.identity_hist[i]) fprintf(f, "  %3d  %llu\n", i, u(e.identity_hist[i]));
	fprintf(f, "alternative references per edit-script read: mean %.4f (distinct alternatives: reads):\n", D.alts_per_read);
	for (int i = 0; i <= 64; ++i) if (e.alt_hist[i]) fprintf(f, "  %2d  %llu\n", i, u(e.alt_hist[i]));
}
// the whole stream as one JSON object, the derived values behind it
inline void print_edits_json(FILE* f, const EditsSet& S)
{
	const cl_edits& e = *S.e; const EditsDerived D = edits_derived(e);
	auto arr = [&](const char* name, const uint64_t* p, int n) { fprintf(f, ", \"%s\": [", name); for (int i = 0; i < n; ++i) fprintf(f, "%s%llu", i ? ", " : "", (unsigned long long)p[i]); fprintf(f, "]"); };
	auto num = [&](const char* name, uint64_t x) { fprintf(f, ", \"%s\": %llu", name, (unsigned long long)x); };
	fprintf(f, "{\"version\": 1, \"flags\": 0, \"note\": \"%s\"", EDITS_NOTE);
	num("reads", e.reads); num("bases", e.bases); arr("kind_reads", e.kind_reads, 3); arr("kind_bases", e.kind_bases, 3); arr("kind_bytes", e.kind_bytes, 3);
	arr("main_rev", e.main_rev, 2); arr("tuples", e.tuples, 8); num("anchor_bases", e.anchor_bases); arr("anchor_len_hist", e.anchor_len_hist, 29);
	num("skip_entries", e.skip_entries); num("skip_entry_sum", e.skip_entry_sum); num("skip_bases", e.skip_bases); arr("skip_len_hist", e.skip_len_hist, 29);
	arr("ins_base", e.ins_base, 4); arr("del_base", e.del_base, 4); arr("match_base", e.match_base, 4);
	fprintf(f, ", \"sub\": [");
	for (int i = 0; i < 4; ++i) fprintf(f, "%s[%llu, %llu, %llu, %llu]", i ? ", " : "", (unsigned long long)e.sub[i][0], (unsigned long long)e.sub[i][1], (unsigned long long)e.sub[i][2], (unsigned long long)e.sub[i][3]);
	fprintf(f, "]");
	arr("ins_run_hist", e.ins_run_hist, 17); arr("del_run_hist", e.del_run_hist, 17); arr("identity_hist", e.identity_hist, 101); num("identity_none", e.identity_none);
	arr("alt_hist", e.alt_hist, 65);
	fprintf(f, ", \"derived\": {\"kind_read_share\": [%.9f, %.9f, %.9f], \"kind_base_share\": [%.9f, %.9f, %.9f], \"anchor_base_share\": %.9f, \"aligned_bases\": %llu, \"sub_rate\": %.9f, \"ins_rate\": %.9f, "
		"\"del_rate\": %.9f, \"transitions\": %llu, \"transversions\": %llu, \"ins_run_mean\": %.9f, \"del_run_mean\": %.9f, \"ins_in_runs2\": %.9f, \"del_in_runs2\": %.9f, \"identity_median\": %d, \"alts_per_read\": %.9f}}\n",
		D.kind_read_share[0], D.kind_read_share[1], D.kind_read_share[2], D.kind_base_share[0], D.kind_base_share[1], D.kind_base_share[2], D.anchor_base_share, (unsigned long long)D.aligned,
		D.sub_rate, D.ins_rate, D.del_rate, (unsigned long long)D.transitions, (unsigned long long)D.transversions, D.ins_run_mean, D.del_run_mean, D.ins_in_runs2, D.del_in_runs2, D.identity_median, D.alts_per_read);
}
