// kspec_stream.hpp — the `hipkmers` stream of an archive: the count spectrum of the sampled k-mers pass 1 counted, taken
// on the device from the sorted keys before the cut at ci (-L) and the saturation at cs (-H) (`colord_hip compress-* --kmer-spectrum`),
// printed by `colord_hip info [--kmer-spectrum [--json]]` without decoding anything.  One part, little-endian, of a fixed size:
//   eight u32: version = 1, flags (bit 0: the k-mers of a reference genome, -G, were counted too), k, f, ci, cs, sets, 0
//   then every word of cl_kspec in its order as u64 (4165 of them)
// sets = the number of independent k-mer sets added: 1 for a plain run, --stream-input and --gpus N (the ranks own disjoint key ranges
// of ONE set), K for --domains K.  Shares and estimates are made when printing and never stored.  The reference's decompressor finds
// its streams by name and never sees this one; `decompress` and `check` do not recompute it.
// WHAT IT IS: the k-mers are the 1-in-f hash sample of the canonical k-mers, so every number is of the sample; the peak is the depth
// of error-free K-MERS, not of bases; the genome size is an estimate.
#pragma once
#include "archive.hpp"
#include "../kspec.hpp"
#include <memory>

struct KSpecSet {
	std::unique_ptr<cl_kspec> s{ new cl_kspec };
	uint32_t flags = 0, k = 0, f = 0, ci = 0, cs = 0, sets = 1;
	KSpecSet() { ks_clear(s.get()); }
	static constexpr size_t BYTES = 32 + 8 * (size_t)KS_WORDS;
	std::vector<uint8_t> pack() const
	{
		std::vector<uint8_t> v; v.reserve(BYTES);
		auto le = [&](uint64_t x, int n) { for (int i = 0; i < n; ++i) v.push_back((uint8_t)(x >> (8 * i))); };
		le(1, 4); le(flags, 4); le(k, 4); le(f, 4); le(ci, 4); le(cs, 4); le(sets, 4); le(0, 4);
		const uint64_t* w = (const uint64_t*)s.get();
		for (uint32_t i = 0; i < KS_WORDS; ++i) le(w[i], 8);
		return v;
	}
	// false: another version, unknown flags, a header this build does not know, another size
	bool unpack(const std::vector<uint8_t>& v)
	{
		ks_clear(s.get());
		if (v.size() != BYTES) return false;
		auto le = [&](size_t at, int n) { uint64_t x = 0; for (int i = 0; i < n; ++i) x |= (uint64_t)v[at + i] << (8 * i); return x; };
		if (le(0, 4) != 1 || le(4, 4) > 1 || le(28, 4) != 0) return false;
		flags = (uint32_t)le(4, 4); k = (uint32_t)le(8, 4); f = (uint32_t)le(12, 4); ci = (uint32_t)le(16, 4); cs = (uint32_t)le(20, 4); sets = (uint32_t)le(24, 4);
		if (!k || !f || !sets) return false;
		uint64_t* w = (uint64_t*)s.get();
		for (uint32_t i = 0; i < KS_WORDS; ++i) w[i] = le(32 + 8 * (size_t)i, 8);
		return true;
	}
};

// the stored spectrum of an archive: 0 none, 1 read, -1 a `hipkmers` stream this build cannot read
inline int read_hipkmers(const std::string& path, KSpecSet& out)
{
	ArchiveReader ar;
	if (!ar.open(path)) return 0;
	const int s = ar.id("hipkmers");
	std::vector<uint8_t> b; uint64_t meta = 0; int r = 0;
	if (s >= 0) r = ar.part(s, 0, b, meta) && out.unpack(b) ? 1 : -1;
	ar.close();
	return r;
}

// what is made of the spectrum when printing
struct KSpecDerived {
	bool cuts = false;                                  // ci <= 4096 and cs < 4096: the cut sums below are exact (the bins from 4096 on hold no single counts)
	uint64_t below_distinct = 0, below_kmers = 0;       // c < ci: what -L dropped
	double below_distinct_share = 0, below_kmers_share = 0;
	uint64_t above_distinct = 0, saturated_kmers = 0;   // c > cs: how many, and sum of max(c - cs, 0): what -H removed
	uint64_t kept_distinct = 0, kept_kmers = 0;         // sum over c >= ci of h[c] and of min(c, cs) h[c]: the numbers of the `meta` stream
	bool estimates = false;                             // sets == 1 and no genome: one k-mer set of reads alone
	uint32_t valley = 0, peak = 0;                      // 0: none
	uint64_t above_valley_distinct = 0, above_valley_kmers = 0;
	double genome_size = 0;                             // f * above_valley_kmers / peak (0 without a peak)
};
inline KSpecDerived kspec_derived(const KSpecSet& S)
{
	const cl_kspec& s = *S.s; KSpecDerived D;
	auto ratio = [](uint64_t a, uint64_t b) { return b ? (double)a / (double)b : 0.0; };
	uint64_t big = 0, big_mass = 0;
	for (uint32_t b = 0; b < KS_BINS; ++b) { big += s.big[b]; big_mass += s.big_mass[b]; }
	D.cuts = S.ci <= CL_KSPEC_EXACT && S.cs < CL_KSPEC_EXACT;
	if (D.cuts)
	{
		for (uint32_t c = 1; c < CL_KSPEC_EXACT; ++c)
		{
			const uint64_t h = s.exact[c];
			if (c < S.ci) { D.below_distinct += h; D.below_kmers += (uint64_t)c * h; continue; }
			D.kept_distinct += h; D.kept_kmers += (uint64_t)(c < S.cs ? c : S.cs) * h;
			if (c > S.cs) { D.above_distinct += h; D.saturated_kmers += (uint64_t)(c - S.cs) * h; }
		}
		D.kept_distinct += big; D.kept_kmers += (uint64_t)S.cs * big;
		D.above_distinct += big; D.saturated_kmers += big_mass - (uint64_t)S.cs * big;
		D.below_distinct_share = ratio(D.below_distinct, s.distinct); D.below_kmers_share = ratio(D.below_kmers, s.kmers);
	}
	D.estimates = S.sets == 1 && !(S.flags & 1);
	if (D.estimates)
	{
		// valley: the smallest c >= 1 with h[c + 1] >= h[c] among the exact bins; peak: the lowest c > valley that maximises h[c]
		uint32_t valley = 0;
		for (uint32_t c = 1; c + 1 < CL_KSPEC_EXACT; ++c) if (s.exact[c + 1] >= s.exact[c]) { valley = c; break; }
		if (valley)
		{
			uint64_t above = big, mass = big_mass; uint32_t peak = 0;
			for (uint32_t c = valley + 1; c < CL_KSPEC_EXACT; ++c)
			{
				above += s.exact[c]; mass += (uint64_t)c * s.exact[c];
				if (!peak || s.exact[c] > s.exact[peak]) peak = c;
			}
			// a display rule: below 1000 distinct k-mers above the valley a peak is noise
			if (above >= 1000 && peak)
			{
				D.valley = valley; D.peak = peak; D.above_valley_distinct = above; D.above_valley_kmers = mass;
				D.genome_size = (double)S.f * (double)mass / (double)peak;
			}
		}
	}
	return D;
}
inline const char* const KSPEC_NOTE = "the k-mers are the 1-in-f hash sample of the input's canonical k-mers, so every count is of the sample; the peak is the depth of error-free k-mers, not of bases; the genome size is an estimate";
inline void print_kspec(FILE* fo, const KSpecSet& S)
{
	const cl_kspec& s = *S.s; const KSpecDerived D = kspec_derived(S);
	auto u = [](uint64_t x) { return (unsigned long long)x; };
	fprintf(fo, "k-mer count spectrum: %s\n", KSPEC_NOTE);
	fprintf(fo, "k: %u\nf: %u (1-in-%u hash sample)\nci (-L): %u\ncs (-H): %u\nsets: %u\nreference genome counted too: %s\n", S.k, S.f, S.f, S.ci, S.cs, S.sets, (S.flags & 1) ? "yes" : "no");
	fprintf(fo, "sampled k-mers: %llu\ndistinct: %llu\nhighest count: %llu\n", u(s.kmers), u(s.distinct), u(s.max_count));
	fprintf(fo, "distinct k-mers by count (count: distinct k-mers):\n");
	for (uint32_t c = 1; c < CL_KSPEC_EXACT; ++c) if (s.exact[c]) fprintf(fo, "  %4u  %llu\n", c, u(s.exact[c]));
	bool any_big = false; for (uint32_t b = 0; b < KS_BINS; ++b) any_big = any_big || s.big[b] || s.big_mass[b];
	if (any_big)
	{
		fprintf(fo, "counts of 4096 and more by bit length of the count (bits: distinct k-mers, their occurrences):\n");
		for (uint32_t b = 0; b < KS_BINS; ++b) if (s.big[b] || s.big_mass[b]) fprintf(fo, "  %2u  %llu  %llu\n", b, u(s.big[b]), u(s.big_mass[b]));
	}
	if (D.cuts)
	{
		fprintf(fo, "below ci (dropped by -L %u): %llu distinct (%.4f), %llu occurrences (%.4f)\n", S.ci, u(D.below_distinct), D.below_distinct_share, u(D.below_kmers), D.below_kmers_share);
		fprintf(fo, "above cs (flattened by -H %u): %llu distinct, %llu occurrences removed by saturation\n", S.cs, u(D.above_distinct), u(D.saturated_kmers));
		fprintf(fo, "kept: %llu distinct, %llu occurrences counted (the `meta` stream's numbers)\n", u(D.kept_distinct), u(D.kept_kmers));
	}
	else fprintf(fo, "cut shares: not available (ci or cs lies above the exact bins)\n");
	if (!D.estimates) fprintf(fo, "valley, peak and genome size: not estimated (%s)\n", (S.flags & 1) ? "a reference genome's k-mers are in the spectrum" : "the spectrum adds independent k-mer sets");
	else if (!D.peak) fprintf(fo, "valley: none\npeak: none (no valley, or fewer than 1000 distinct k-mers above it)\ngenome size: none\n");
	else
	{
		fprintf(fo, "valley: %u (first count whose successor has no fewer distinct k-mers: below it mostly errors)\n", D.valley);
		fprintf(fo, "peak: %u (depth of error-free k-mers, not of bases; %llu distinct k-mers, %llu occurrences above the valley)\n", D.peak, u(D.above_valley_distinct), u(D.above_valley_kmers));
		fprintf(fo, "genome size: about %.0f (an estimate: f x occurrences above the valley / peak)\n", D.genome_size);
	}
}
// the whole stream as one JSON object, the derived values behind it; integers exactly, the estimate with 17 significant digits
inline void print_kspec_json(FILE* fo, const KSpecSet& S)
{
	const cl_kspec& s = *S.s; const KSpecDerived D = kspec_derived(S);
	auto u = [](uint64_t x) { return (unsigned long long)x; };
	fprintf(fo, "{\"version\": 1, \"flags\": %u, \"k\": %u, \"f\": %u, \"ci\": %u, \"cs\": %u, \"sets\": %u, \"note\": \"%s\"", S.flags, S.k, S.f, S.ci, S.cs, S.sets, KSPEC_NOTE);
	fprintf(fo, ", \"kmers\": %llu, \"distinct\": %llu, \"max_count\": %llu", u(s.kmers), u(s.distinct), u(s.max_count));
	auto rows = [&](const char* name, const uint64_t* p, uint32_t n, const uint64_t* also) {
		fprintf(fo, ", \"%s\": {", name); bool first = true;
		for (uint32_t i = 0; i < n; ++i) if (p[i] || (also && also[i])) { fprintf(fo, "%s\"%u\": %llu", first ? "" : ", ", i, u(p[i])); first = false; }
		fprintf(fo, "}");
	};
	rows("exact", s.exact, CL_KSPEC_EXACT, nullptr); rows("big", s.big, KS_BINS, s.big_mass); rows("big_mass", s.big_mass, KS_BINS, s.big);
	fprintf(fo, ", \"derived\": {");
	if (D.cuts) fprintf(fo, "\"below_ci_distinct\": %llu, \"below_ci_kmers\": %llu, \"below_ci_distinct_share\": %.12g, \"below_ci_kmers_share\": %.12g, \"above_cs_distinct\": %llu, \"saturated_kmers\": %llu, "
		"\"kept_distinct\": %llu, \"kept_kmers\": %llu, ", u(D.below_distinct), u(D.below_kmers), D.below_distinct_share, D.below_kmers_share, u(D.above_distinct), u(D.saturated_kmers), u(D.kept_distinct), u(D.kept_kmers));
	fprintf(fo, "\"estimates\": %s", D.estimates ? "true" : "false");
	if (D.estimates)
	{
		if (D.peak) fprintf(fo, ", \"valley\": %u, \"peak\": %u, \"above_valley_distinct\": %llu, \"above_valley_kmers\": %llu, \"genome_size\": %.17g", D.valley, D.peak, u(D.above_valley_distinct), u(D.above_valley_kmers), D.genome_size);
		else fprintf(fo, ", \"valley\": null, \"peak\": null, \"genome_size\": null");
	}
	fprintf(fo, "}}\n");
}
