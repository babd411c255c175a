// sketch_stream.hpp — the `hipsketch` stream of an archive: a bottom-s MinHash sketch of the sampled k-mers pass 1 counted
// at least min_count times, made on the device from the sorted keys (`colord_hip compress-* --sketch`), printed by `colord_hip info
// [--sketch [--json]]` and compared by `colord_hip dist` without decoding anything.  One part, little-endian:
//   eight u32: version = 1, flags (bit 0: the k-mers of a reference genome, -G, were counted too), k, f, min_count, size, sets, 0
//   then u64 qualifying, u64 n
//   then n x (u64 hash, u64 count), the hashes strictly ascending, no count 0
// sets = the number of independent k-mer sets merged: 1 for a plain run, --stream-input and --gpus N (the ranks own disjoint key ranges
// of ONE set), K for --domains K — min_count then applied per set and qualifying is a sum over the sets.  n < size: the sketch is
// COMPLETE, it holds every qualifying k-mer (with one set, n == qualifying then).  The reference's decompressor finds its streams by
// name and never sees this one; `decompress` and `check` ignore it.
// WHAT IT IS: the k-mers are the 1-in-f hash sample of the canonical k-mers of noisy reads with count >= min_count, so sketches compare
// at equal k and f only, and a distance from them is not comparable with Mash distances of assembled genomes.
#pragma once
#include "archive.hpp"
#include "../sketch.hpp"
#include <cmath>

struct SketchSet {
	uint32_t flags = 0, k = 0, f = 0, min_count = 0, size = 0, sets = 1;
	uint64_t qualifying = 0;
	std::vector<cl_sketch_entry> e;
	std::vector<uint8_t> pack() const
	{
		std::vector<uint8_t> v; v.reserve(48 + 16 * e.size());
		auto le = [&](uint64_t x, int n) { for (int i = 0; i < n; ++i) v.push_back((uint8_t)(x >> (8 * i))); };
		le(1, 4); le(flags, 4); le(k, 4); le(f, 4); le(min_count, 4); le(size, 4); le(sets, 4); le(0, 4);
		le(qualifying, 8); le(e.size(), 8);
		for (const cl_sketch_entry& x : e) { le(x.hash, 8); le(x.count, 8); }
		return v;
	}
	// false: another version, unknown flags, a header this build does not know, entries that are no sketch, another length
	bool unpack(const std::vector<uint8_t>& v)
	{
		e.clear();
		if (v.size() < 48) return false;
		auto le = [&](size_t at, int n) { uint64_t x = 0; for (int i = 0; i < n; ++i) x |= (uint64_t)v[at + i] << (8 * i); return x; };
		if (le(0, 4) != 1 || le(4, 4) > 1 || le(28, 4) != 0) return false;
		flags = (uint32_t)le(4, 4); k = (uint32_t)le(8, 4); f = (uint32_t)le(12, 4); min_count = (uint32_t)le(16, 4); size = (uint32_t)le(20, 4); sets = (uint32_t)le(24, 4);
		qualifying = le(32, 8); const uint64_t n = le(40, 8);
		if (!k || !f || !sets || !sk_params_ok(size, min_count)) return false;
		if (n > size || (n < size && n != qualifying && sets == 1)) return false;
		if (v.size() != 48 + 16 * n) return false;
		e.resize(n);
		for (uint64_t i = 0; i < n; ++i) { e[i].hash = le(48 + 16 * i, 8); e[i].count = le(56 + 16 * i, 8); }
		if (!sk_entries_ok(e.data(), n)) { e.clear(); return false; }
		return true;
	}
	bool complete() const { return e.size() < size; }
	// (n - 1) 2^64 / hash[n - 1]: the cardinality estimate of a bottom-n sketch; 0 where there is none
	double cardinality() const { return e.size() >= 2 && e.back().hash ? (double)(e.size() - 1) * 18446744073709551616.0 / (double)e.back().hash : 0.0; }
};

// the stored sketch of an archive: 0 none, 1 read, -1 a `hipsketch` stream this build cannot read
inline int read_hipsketch(const std::string& path, SketchSet& out)
{
	ArchiveReader ar;
	if (!ar.open(path)) return 0;
	const int s = ar.id("hipsketch");
	std::vector<uint8_t> b; uint64_t meta = 0; int r = 0;
	if (s >= 0) r = ar.part(s, 0, b, meta) && out.unpack(b) ? 1 : -1;
	ar.close();
	return r;
}

inline const char* const SKETCH_NOTE = "a bottom-s MinHash sketch of the 1-in-f hash sample of the input's canonical k-mers that occur at least min_count times in the reads; "
	"sketches compare at equal k and f only; it is no sketch of an assembly, so its distance is not comparable with Mash distances of genomes";
inline const char* const SKETCH_SETS_NOTE = "independent k-mer sets were merged: min_count applied per set, and qualifying is a sum over the sets";
inline void print_sketch(FILE* fo, const SketchSet& S)
{
	auto u = [](uint64_t x) { return (unsigned long long)x; };
	fprintf(fo, "k-mer sketch: %s\n", SKETCH_NOTE);
	fprintf(fo, "k: %u\nf: %u (1-in-%u hash sample)\nmin_count: %u\nsize: %u\nsets: %u%s%s%s\nreference genome counted too: %s\n", S.k, S.f, S.f, S.min_count, S.size, S.sets,
		S.sets > 1 ? " (" : "", S.sets > 1 ? SKETCH_SETS_NOTE : "", S.sets > 1 ? ")" : "", (S.flags & 1) ? "yes" : "no");
	fprintf(fo, "qualifying: %llu\nentries: %llu\n", u(S.qualifying), u(S.e.size()));
	if (S.complete()) fprintf(fo, "complete: yes (it holds every qualifying k-mer)\n");
	else fprintf(fo, "complete: no (the %u lowest hashes; cardinality estimate %.0f beside qualifying %llu)\n", S.size, S.cardinality(), u(S.qualifying));
	if (!S.e.empty()) fprintf(fo, "lowest hash: %llu\nhighest hash: %llu\n", u(S.e.front().hash), u(S.e.back().hash));
}
// the whole stream as one JSON object; integers exactly, the estimate with 17 significant digits
inline void print_sketch_json(FILE* fo, const SketchSet& S)
{
	auto u = [](uint64_t x) { return (unsigned long long)x; };
	fprintf(fo, "{\"version\": 1, \"flags\": %u, \"k\": %u, \"f\": %u, \"min_count\": %u, \"size\": %u, \"sets\": %u, \"note\": \"%s\"", S.flags, S.k, S.f, S.min_count, S.size, S.sets, SKETCH_NOTE);
	fprintf(fo, ", \"qualifying\": %llu, \"n\": %llu, \"complete\": %s", u(S.qualifying), u(S.e.size()), S.complete() ? "true" : "false");
	if (!S.complete()) fprintf(fo, ", \"cardinality_estimate\": %.17g", S.cardinality());
	fprintf(fo, ", \"hash\": [");
	for (size_t i = 0; i < S.e.size(); ++i) fprintf(fo, "%s%llu", i ? ", " : "", u(S.e[i].hash));
	fprintf(fo, "], \"count\": [");
	for (size_t i = 0; i < S.e.size(); ++i) fprintf(fo, "%s%llu", i ? ", " : "", u(S.e[i].count));
	fprintf(fo, "]}\n");
}

// a path as the inside of a JSON string
inline std::string json_escape(const std::string& s)
{
	std::string o;
	for (const unsigned char c : s)
	{
		if (c == '"' || c == '\\') { o.push_back('\\'); o.push_back((char)c); }
		else if (c < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", c); o += b; }
		else o.push_back((char)c);
	}
	return o;
}

// `colord_hip dist`: two sketches of equal k and f compared up to the threshold both cover
struct SketchDist { uint64_t shared = 0, compared = 0, in_a = 0, in_b = 0; double jaccard = 0, containment_a = 0, containment_b = 0, distance = 1; };
inline SketchDist sketch_dist(const SketchSet& A, const SketchSet& B)
{
	// T_X: the largest hash of X if X is full, else 2^64 - 1 (X then holds every qualifying k-mer)
	auto top = [](const SketchSet& X) { return X.e.size() == X.size ? X.e.back().hash : ~0ULL; };
	const uint64_t T = std::min(top(A), top(B));
	SketchDist D; size_t a = 0, b = 0;
	while ((a < A.e.size() && A.e[a].hash <= T) || (b < B.e.size() && B.e[b].hash <= T))
	{
		const bool ha = a < A.e.size() && A.e[a].hash <= T, hb = b < B.e.size() && B.e[b].hash <= T;
		++D.compared;
		if (ha && hb && A.e[a].hash == B.e[b].hash) { ++D.shared; ++D.in_a; ++D.in_b; ++a; ++b; }
		else if (ha && (!hb || A.e[a].hash < B.e[b].hash)) { ++D.in_a; ++a; }
		else { ++D.in_b; ++b; }
	}
	D.jaccard = D.compared ? (double)D.shared / (double)D.compared : 0.0;
	D.containment_a = D.in_a ? (double)D.shared / (double)D.in_a : 0.0;
	D.containment_b = D.in_b ? (double)D.shared / (double)D.in_b : 0.0;
	const double j = D.jaccard;
	D.distance = (D.compared && D.shared == D.compared) ? 0.0 : !D.shared ? 1.0 : -std::log(2.0 * j / (1.0 + j)) / (double)A.k;
	return D;
}
