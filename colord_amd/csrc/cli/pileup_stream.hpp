// pileup_stream.hpp — the `hippileup` stream of an archive: the SITES of the per-position base counts of a reference-genome run
// (`colord_hip compress-* -G genome.fa --pileup`): the positions of the genome at which enough read columns say something else than the genome,
// printed by `colord_hip info --pileup` as a table, as a minimal VCF or as a summary without decoding `dna` or `qual` and without a GPU.
// THE FULL TABLE IS NOT STORED: it is the size of the genome (32 bytes per position); the stream holds its totals and its sites.
// One part, little-endian:
//   u32 version = 1, u32 record size = 48, u32 n_seqs, u32 read_len, u32 overlap (the pieces' geometry),
//   u32 min_depth, u32 min_alt, u32 min_permille (the thresholds the sites were taken with),
//   7 x u64 totals (cl_pileup_sums: covered positions, match, sub, del, ins, insertion runs without a position, reads on genome pieces), u64 count,
//   per sequence: u64 length (the kept bases), u16 name length, the name (the FASTA header behind `>` up to the first blank),
//   then `count` sites of twelve u32 (cl_pileup_site: seq, pos, ref, kind, match, sub A C G T, del, ins, depth) in genome order
// The reference's decompressor finds its streams by name and never sees this one; `decompress` and `check` ignore it.
#pragma once
#include "archive.hpp"
#include "../pileup.hpp"
#include <algorithm>
#include <string>

struct PileupSet {
	uint32_t read_len = 0, overlap = 0; PileThresholds thr{ 0, 0, 0 };
	cl_pileup_sums sums{};
	std::vector<uint64_t> seq_len; std::vector<std::string> names;             // per sequence of the genome, as read_fasta indexes them
	std::vector<cl_pileup_site> sites;
	static constexpr uint32_t VERSION = 1, RECORD_BYTES = PU_SITE_WORDS * 4;
	static constexpr size_t HEAD = 32 + PU_SUMS * 8 + 8;
	static void words(const cl_pileup_site& o, uint32_t* w) { const uint32_t v[PU_SITE_WORDS] = { o.seq, o.pos, o.ref, o.kind, o.match, o.sub[0], o.sub[1], o.sub[2], o.sub[3], o.del, o.ins, o.depth }; std::copy(v, v + PU_SITE_WORDS, w); }
	std::vector<uint8_t> pack() const
	{
		std::vector<uint8_t> v; v.reserve(HEAD + seq_len.size() * 32 + sites.size() * RECORD_BYTES);
		auto le = [&](uint64_t x, int n) { for (int i = 0; i < n; ++i) v.push_back((uint8_t)(x >> (8 * i))); };
		le(VERSION, 4); le(RECORD_BYTES, 4); le(seq_len.size(), 4); le(read_len, 4); le(overlap, 4); le(thr.min_depth, 4); le(thr.min_alt, 4); le(thr.min_permille, 4);
		const uint64_t t[PU_SUMS] = { sums.covered, sums.match, sums.sub, sums.del, sums.ins, sums.ins_unplaced, sums.reads };
		for (uint64_t x : t) le(x, 8);
		le(sites.size(), 8);
		for (size_t s = 0; s < seq_len.size(); ++s)
		{
			const std::string nm = names[s].substr(0, 0xffff);
			le(seq_len[s], 8); le(nm.size(), 2); v.insert(v.end(), nm.begin(), nm.end());
		}
		for (const cl_pileup_site& o : sites) { uint32_t w[PU_SITE_WORDS]; words(o, w); for (uint32_t x : w) le(x, 4); }
		return v;
	}
	// false: another version, another record size, a name table or a count that is not what the bytes hold, a site on a sequence the table does
	// not hold or behind its end, a reference base or a kind out of range (the kind is never the reference base), sites that are not in genome order
	bool unpack(const std::vector<uint8_t>& v)
	{
		sites.clear(); seq_len.clear(); names.clear();
		if (v.size() < HEAD) return false;
		auto le = [&](size_t at, int n) { uint64_t x = 0; for (int i = 0; i < n; ++i) x |= (uint64_t)v[at + i] << (8 * i); return x; };
		if (le(0, 4) != VERSION || le(4, 4) != RECORD_BYTES) return false;
		const uint64_t n_seqs = le(8, 4), n = le(HEAD - 8, 8);
		read_len = (uint32_t)le(12, 4); overlap = (uint32_t)le(16, 4); thr = PileThresholds{ (uint32_t)le(20, 4), (uint32_t)le(24, 4), (uint32_t)le(28, 4) };
		uint64_t t[PU_SUMS]; for (uint32_t i = 0; i < PU_SUMS; ++i) t[i] = le(32 + 8 * (size_t)i, 8);
		sums = cl_pileup_sums{ t[0], t[1], t[2], t[3], t[4], t[5], t[6] };
		size_t at = HEAD;
		if (n_seqs > (v.size() - at) / 10) return false;                       // (an entry is ten bytes at the least: nothing is reserved for a count the bytes cannot hold)
		for (uint64_t s = 0; s < n_seqs; ++s)
		{
			if (v.size() - at < 10) return false;
			const uint64_t len = le(at, 8); const size_t nl = (size_t)le(at + 8, 2);
			at += 10;
			if (v.size() - at < nl) return false;
			seq_len.push_back(len); names.emplace_back((const char*)v.data() + at, nl);
			at += nl;
		}
		if ((v.size() - at) % RECORD_BYTES || (v.size() - at) / RECORD_BYTES != n) return false;
		sites.resize(n);
		for (uint64_t i = 0; i < n; ++i)
		{
			uint32_t w[PU_SITE_WORDS];
			for (uint32_t k = 0; k < PU_SITE_WORDS; ++k) w[k] = (uint32_t)le(at + i * RECORD_BYTES + 4 * (size_t)k, 4);
			cl_pileup_site& o = sites[i];
			o.seq = w[0]; o.pos = w[1]; o.ref = w[2]; o.kind = w[3]; o.match = w[4]; o.sub[0] = w[5]; o.sub[1] = w[6]; o.sub[2] = w[7]; o.sub[3] = w[8]; o.del = w[9]; o.ins = w[10]; o.depth = w[11];
			const bool ordered = !i || sites[i - 1].seq < o.seq || (sites[i - 1].seq == o.seq && sites[i - 1].pos < o.pos);
			if (o.seq >= n_seqs || o.pos >= seq_len[o.seq] || o.ref > 3 || o.kind > PU_KIND_INS || o.kind == o.ref || !ordered) { sites.clear(); return false; }
		}
		return true;
	}
	// the name a sequence is printed by: its FASTA name, or its index where the header line holds none
	std::string name_of(uint32_t s) const { return names[s].empty() ? std::to_string(s) : names[s]; }
};

// the stored pileup of an archive: 0 none, 1 read, -1 a `hippileup` stream this build cannot read
inline int read_hippileup(const std::string& path, PileupSet& out)
{
	ArchiveReader ar;
	if (!ar.open(path)) return 0;
	const int s = ar.id("hippileup");
	std::vector<uint8_t> b; uint64_t meta = 0; int r = 0;
	if (s >= 0) r = ar.part(s, 0, b, meta) && out.unpack(b) ? 1 : -1;
	ar.close();
	return r;
}

// the columns that say a site's alternative
inline uint32_t pileup_alt(const cl_pileup_site& o) { return o.kind < 4 ? o.sub[o.kind] : o.kind == PU_KIND_DEL ? o.del : o.ins; }
// thresholds given to `info` can only tighten what was stored
inline bool pileup_keeps(const cl_pileup_site& o, uint64_t min_alt, uint64_t min_permille) { const uint64_t a = pileup_alt(o); return a >= min_alt && a * 1000 >= min_permille * o.depth; }
inline const char* pileup_kind_name(uint32_t k) { static const char* const T[6] = { "A", "C", "G", "T", "del", "ins" }; return k < 6 ? T[k] : "?"; }

// a line per site: sequence name, 1-based position, the genome's base, depth, the columns that say A, C, G, T (the reference base's is `match`),
// deletions, insertion runs left of which the position lies, the kind of the alternative
inline void print_pileup_table(FILE* f, const PileupSet& S, uint64_t min_alt, uint64_t min_permille)
{
	for (const cl_pileup_site& o : S.sites)
	{
		if (!pileup_keeps(o, min_alt, min_permille)) continue;
		uint32_t b[4]; for (uint32_t k = 0; k < 4; ++k) b[k] = k == o.ref ? o.match : o.sub[k];
		fprintf(f, "%s\t%llu\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%s\n", S.name_of(o.seq).c_str(), (unsigned long long)o.pos + 1, "ACGT"[o.ref], o.depth, b[0], b[1], b[2], b[3], o.del, o.ins, pileup_kind_name(o.kind));
	}
}
// a minimal VCF 4.2 of the sites whose alternative is a base: no genotype column
inline void print_pileup_vcf(FILE* f, const PileupSet& S, uint64_t min_alt, uint64_t min_permille)
{
	fprintf(f, "##fileformat=VCFv4.2\n##source=colord_hip\n");
	for (size_t s = 0; s < S.seq_len.size(); ++s) fprintf(f, "##contig=<ID=%s,length=%llu>\n", S.name_of((uint32_t)s).c_str(), (unsigned long long)S.seq_len[s]);
	fprintf(f, "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Aligned columns at the position: match + substitutions + deletions\">\n"
		"##INFO=<ID=AD,Number=R,Type=Integer,Description=\"Columns that say the reference base, columns that say the alternative\">\n"
		"##INFO=<ID=AF,Number=A,Type=Float,Description=\"Alternative columns over DP\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n");
	for (const cl_pileup_site& o : S.sites)
		if (o.kind < 4 && pileup_keeps(o, min_alt, min_permille))
			fprintf(f, "%s\t%llu\t.\t%c\t%c\t.\t.\tDP=%u;AD=%u,%u;AF=%.4f\n", S.name_of(o.seq).c_str(), (unsigned long long)o.pos + 1, "ACGT"[o.ref], "ACGT"[o.kind], o.depth, o.match, o.sub[o.kind],
				o.depth ? (double)o.sub[o.kind] / (double)o.depth : 0.0);
}
// the totals, the mean depth over covered positions, the rates per aligned column, the sites per kind
inline void print_pileup_summary(FILE* f, const PileupSet& S, bool json)
{
	auto u = [](uint64_t x) { return (unsigned long long)x; };
	const cl_pileup_sums& t = S.sums;
	const uint64_t cols = t.match + t.sub + t.del;
	uint64_t positions = 0, by[6] = { 0 };
	for (uint64_t l : S.seq_len) positions += l;
	for (const cl_pileup_site& o : S.sites) ++by[o.kind];
	auto rate = [](uint64_t a, uint64_t b) { return b ? (double)a / (double)b : 0.0; };
	if (json)
	{
		fprintf(f, "{\"sequences\": %zu, \"positions\": %llu, \"min_depth\": %u, \"min_alt\": %u, \"min_permille\": %u, \"covered\": %llu, \"match\": %llu, \"sub\": %llu, \"del\": %llu, \"ins\": %llu, \"ins_unplaced\": %llu, "
			"\"reads\": %llu, \"mean_depth\": %.6f, \"sub_rate\": %.6f, \"del_rate\": %.6f, \"ins_rate\": %.6f, \"sites\": %zu, \"sites_by_kind\": {", S.seq_len.size(), u(positions), S.thr.min_depth, S.thr.min_alt,
			S.thr.min_permille, u(t.covered), u(t.match), u(t.sub), u(t.del), u(t.ins), u(t.ins_unplaced), u(t.reads), rate(cols, t.covered), rate(t.sub, cols), rate(t.del, cols), rate(t.ins, cols), S.sites.size());
		for (uint32_t k = 0; k < 6; ++k) fprintf(f, "%s\"%s\": %llu", k ? ", " : "", pileup_kind_name(k), u(by[k]));
		fprintf(f, "}}\n");
		return;
	}
	fprintf(f, "sequences: %zu\npositions: %llu\npositions with an aligned column: %llu\nreads on genome pieces: %llu\nmatch columns: %llu\nsubstitution columns: %llu\ndeletion columns: %llu\n"
		"insertion runs: %llu (and %llu without a position)\nmean depth over covered positions: %.6f\nper aligned column: substitutions %.6f, deletions %.6f, insertion runs %.6f\n"
		"sites (depth >= %u, alternative >= %u columns and >= %u permille of the depth): %zu\n", S.seq_len.size(), u(positions), u(t.covered), u(t.reads), u(t.match), u(t.sub), u(t.del), u(t.ins), u(t.ins_unplaced),
		rate(cols, t.covered), rate(t.sub, cols), rate(t.del, cols), rate(t.ins, cols), S.thr.min_depth, S.thr.min_alt, S.thr.min_permille, S.sites.size());
	for (uint32_t k = 0; k < 6; ++k) fprintf(f, "  %s: %llu\n", pileup_kind_name(k), u(by[k]));
}
