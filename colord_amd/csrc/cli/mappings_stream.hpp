// mappings_stream.hpp — the `hipmappings` stream of an archive: the read-to-genome alignments of a reference-genome run
// (`colord_hip compress-* -G genome.fa --mappings`), one record per stretch of a read's edit script on one PIECE of the genome, lifted on the
// device to the coordinates of the genome's sequences, printed by `colord_hip info --mappings` as PAF, as a windowed coverage track or as a
// summary without decoding `dna` or `qual` and without a GPU.  One part, little-endian:
//   u32 version = 1, u32 record size = 48, u32 n_seqs, u32 read_len, u32 overlap (the pieces' geometry), u64 count,
//   per sequence: u64 length (the kept bases), u16 name length, the name (the FASTA header behind `>` up to the first blank),
//   then `count` records of twelve u32 (cl_overlap: t = the sequence, ts / te its coordinates, flags bit 2 set), reads in input order
// The records are stored as they are.  The reference's decompressor finds its streams by name and never sees this one; `decompress` and
// `check` ignore it.
// WHAT IT IS NOT: a read coded against earlier reads instead of genome pieces yields no record, and a read that spans a piece boundary yields
// one record per piece; these are not stitched.
#pragma once
#include "archive.hpp"
#include "../mappings.hpp"
#include <algorithm>
#include <string>

struct MappingSet {
	uint32_t read_len = 0, overlap = 0;
	std::vector<uint64_t> seq_len; std::vector<std::string> names;             // per sequence of the genome, as read_fasta indexes them
	std::vector<cl_overlap> recs;
	static constexpr uint32_t VERSION = 1, RECORD_BYTES = OV_WORDS * 4;
	static constexpr size_t HEAD = 28;
	std::vector<uint8_t> pack() const
	{
		std::vector<uint8_t> v; v.reserve(HEAD + seq_len.size() * 32 + recs.size() * RECORD_BYTES);
		auto le = [&](uint64_t x, int n) { for (int i = 0; i < n; ++i) v.push_back((uint8_t)(x >> (8 * i))); };
		le(VERSION, 4); le(RECORD_BYTES, 4); le(seq_len.size(), 4); le(read_len, 4); le(overlap, 4); le(recs.size(), 8);
		for (size_t s = 0; s < seq_len.size(); ++s)
		{
			const std::string nm = names[s].substr(0, 0xffff);
			le(seq_len[s], 8); le(nm.size(), 2); v.insert(v.end(), nm.begin(), nm.end());
		}
		for (const cl_overlap& o : recs) { const uint32_t w[OV_WORDS] = { o.q, o.t, o.qlen, o.tlen, o.qs, o.qe, o.ts, o.te, o.matches, o.subst, o.anchor_bases, o.flags }; for (uint32_t x : w) le(x, 4); }
		return v;
	}
	// false: another version, another record size, a name table or a count that is not what the bytes hold, a record that names a sequence the
	// table does not hold or that ends behind its sequence
	bool unpack(const std::vector<uint8_t>& v)
	{
		recs.clear(); seq_len.clear(); names.clear();
		if (v.size() < HEAD) return false;
		auto le = [&](size_t at, int n) { uint64_t x = 0; for (int i = 0; i < n; ++i) x |= (uint64_t)v[at + i] << (8 * i); return x; };
		if (le(0, 4) != VERSION || le(4, 4) != RECORD_BYTES) return false;
		const uint64_t n_seqs = le(8, 4), n = le(20, 8);
		read_len = (uint32_t)le(12, 4); overlap = (uint32_t)le(16, 4);
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
		recs.resize(n);
		for (uint64_t i = 0; i < n; ++i)
		{
			uint32_t w[OV_WORDS];
			for (uint32_t k = 0; k < OV_WORDS; ++k) w[k] = (uint32_t)le(at + i * RECORD_BYTES + 4 * (size_t)k, 4);
			cl_overlap& o = recs[i];
			o.q = w[0]; o.t = w[1]; o.qlen = w[2]; o.tlen = w[3]; o.qs = w[4]; o.qe = w[5]; o.ts = w[6]; o.te = w[7]; o.matches = w[8]; o.subst = w[9]; o.anchor_bases = w[10]; o.flags = w[11];
			if (o.t >= n_seqs || o.te > seq_len[o.t]) { recs.clear(); return false; }
		}
		return true;
	}
	// the name a sequence is printed by: its FASTA name, or its index where the header line holds none
	std::string name_of(uint32_t s) const { return names[s].empty() ? std::to_string(s) : names[s]; }
};

// the stored mappings of an archive: 0 none, 1 read, -1 a `hipmappings` stream this build cannot read
inline int read_hipmappings(const std::string& path, MappingSet& out)
{
	ArchiveReader ar;
	if (!ar.open(path)) return 0;
	const int s = ar.id("hipmappings");
	std::vector<uint8_t> b; uint64_t meta = 0; int r = 0;
	if (s >= 0) r = ar.part(s, 0, b, meta) && out.unpack(b) ? 1 : -1;
	ar.close();
	return r;
}

// PAF, a line per record whose block length is at least min_block: query, qlen, qs, qe, strand, the target SEQUENCE's name, its length, ts, te,
// matches, block, 255, then mm:i: (subst), an:i: (anchor bases), tp:A:P (the read's main reference) or tp:A:S (an alternative).  names (or
// null): the id of every read of the input; without them a read's name is its index.  false: a record names a read the names do not hold.
inline bool print_mappings_paf(FILE* f, const MappingSet& S, uint64_t min_block, const std::vector<std::string>* names)
{
	for (const cl_overlap& o : S.recs)
	{
		const uint64_t blk = ov_block(o);
		if (blk < min_block) continue;
		if (names && o.q >= names->size()) return false;
		const std::string q = names ? (*names)[o.q] : std::to_string(o.q);
		fprintf(f, "%s\t%u\t%u\t%u\t%c\t%s\t%llu\t%u\t%u\t%u\t%llu\t255\tmm:i:%u\tan:i:%u\ttp:A:%c\n", q.c_str(), o.qlen, o.qs, o.qe, (o.flags & OV_REV) ? '-' : '+', S.name_of(o.t).c_str(),
			(unsigned long long)S.seq_len[o.t], o.ts, o.te, o.matches, (unsigned long long)blk, o.subst, o.anchor_bases, (o.flags & OV_MAIN) ? 'P' : 'S');
	}
	return true;
}

// bedGraph, a line per window of `window` bases of every sequence (the last window of a sequence is short): name, start, end, the mean depth —
// the target bases [ts, te) of the records that fall into the window over the window's length.  On the host: the records are a few bytes per read.
inline void print_mappings_coverage(FILE* f, const MappingSet& S, uint64_t window)
{
	std::vector<std::vector<uint64_t>> sum(S.seq_len.size());
	for (size_t s = 0; s < S.seq_len.size(); ++s) sum[s].assign((size_t)((S.seq_len[s] + window - 1) / window), 0);
	for (const cl_overlap& o : S.recs)                                        // (t < n_seqs and ts <= te <= its length: unpack, and the loop below needs no more)
		for (uint64_t a = o.ts; a < o.te;)
		{
			const uint64_t w = a / window, e = std::min<uint64_t>((w + 1) * window, o.te);
			sum[o.t][(size_t)w] += e - a;
			a = e;
		}
	for (size_t s = 0; s < S.seq_len.size(); ++s)
		for (size_t w = 0; w < sum[s].size(); ++w)
		{
			const uint64_t a = (uint64_t)w * window, e = std::min<uint64_t>(a + window, S.seq_len[s]);
			fprintf(f, "%s\t%llu\t%llu\t%.6f\n", S.name_of((uint32_t)s).c_str(), (unsigned long long)a, (unsigned long long)e, (double)sum[s][w] / (double)(e - a));
		}
}

// what the records add up to; n_reads: the reads of the archive
struct MappingSummary { uint64_t reads = 0, reads_mapped = 0, records = 0, aligned_query_bases = 0, forward = 0, reverse = 0, identity_hist[101] = { 0 }; };
inline MappingSummary summarize_mappings(const MappingSet& S, uint64_t n_reads)
{
	MappingSummary M; M.reads = n_reads; M.records = S.recs.size();
	std::vector<uint32_t> qs;
	for (const cl_overlap& o : S.recs)
	{
		qs.push_back(o.q);
		M.aligned_query_bases += o.qe >= o.qs ? o.qe - o.qs : 0;
		++((o.flags & OV_REV) ? M.reverse : M.forward);
		const uint64_t blk = ov_block(o), m = std::min<uint64_t>(o.matches, blk);   // identity = matches / block, in bins of one percent (100: all of it)
		++M.identity_hist[blk ? 100 * m / blk : 0];
	}
	std::sort(qs.begin(), qs.end());
	M.reads_mapped = (uint64_t)(std::unique(qs.begin(), qs.end()) - qs.begin());
	return M;
}
inline void print_mappings_summary(FILE* f, const MappingSummary& M, bool json)
{
	auto u = [](uint64_t x) { return (unsigned long long)x; };
	if (json)
	{
		fprintf(f, "{\"reads\": %llu, \"reads_mapped\": %llu, \"records\": %llu, \"aligned_query_bases\": %llu, \"forward\": %llu, \"reverse\": %llu, \"identity_hist\": [", u(M.reads), u(M.reads_mapped), u(M.records),
			u(M.aligned_query_bases), u(M.forward), u(M.reverse));
		for (int i = 0; i <= 100; ++i) fprintf(f, "%s%llu", i ? ", " : "", u(M.identity_hist[i]));
		fprintf(f, "]}\n");
		return;
	}
	fprintf(f, "reads in the archive: %llu\nreads with a mapping: %llu\nrecords: %llu\naligned query bases: %llu\nforward strand: %llu\nreverse strand: %llu\nidentity (matches / block) of the records, in percent:\n",
		u(M.reads), u(M.reads_mapped), u(M.records), u(M.aligned_query_bases), u(M.forward), u(M.reverse));
	for (int i = 0; i <= 100; ++i) if (M.identity_hist[i]) fprintf(f, "  %3d: %llu\n", i, u(M.identity_hist[i]));
}
