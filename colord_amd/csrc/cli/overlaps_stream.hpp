// overlaps_stream.hpp — the `hipoverlaps` stream of an archive: the read-to-read overlaps the edit scripts hold, one record per
// visit of a read on a reference read, made on the device right behind the edit scripts (`colord_hip compress-* --overlaps`) and printed as
// PAF by `colord_hip info --overlaps [--min-block N] [--names]` without decoding `dna` or `qual`.  One part, little-endian:
//   u32 version = 1, u32 record size = 48, u64 count, then `count` records of twelve u32 (cl_overlap), reads in input order
// The records are stored as they are (a compressed form is a later step).  The reference's decompressor finds its streams by name and never
// sees this one; `decompress` and `check` ignore it.
// WHAT IT IS: a read against earlier READS, which carry errors of their own, and overlaps with REFERENCE reads only — about a tenth of the
// reads with the sparse acceptor, all of them otherwise.
#pragma once
#include "archive.hpp"
#include "../overlaps.hpp"

struct OverlapSet {
	std::vector<cl_overlap> recs;
	static constexpr uint32_t VERSION = 1, RECORD_BYTES = OV_WORDS * 4;
	static constexpr size_t HEAD = 16;
	std::vector<uint8_t> pack() const
	{
		std::vector<uint8_t> v; v.reserve(HEAD + recs.size() * RECORD_BYTES);
		auto le = [&](uint64_t x, int n) { for (int i = 0; i < n; ++i) v.push_back((uint8_t)(x >> (8 * i))); };
		le(VERSION, 4); le(RECORD_BYTES, 4); le(recs.size(), 8);
		for (const cl_overlap& o : recs) { const uint32_t w[OV_WORDS] = { o.q, o.t, o.qlen, o.tlen, o.qs, o.qe, o.ts, o.te, o.matches, o.subst, o.anchor_bases, o.flags }; for (uint32_t x : w) le(x, 4); }
		return v;
	}
	// false: another version, another record size, a count that is not what the bytes hold (a truncated stream)
	bool unpack(const std::vector<uint8_t>& v)
	{
		recs.clear();
		if (v.size() < HEAD) return false;
		auto le = [&](size_t at, int n) { uint64_t x = 0; for (int i = 0; i < n; ++i) x |= (uint64_t)v[at + i] << (8 * i); return x; };
		if (le(0, 4) != VERSION || le(4, 4) != RECORD_BYTES) return false;
		const uint64_t n = le(8, 8);
		if ((v.size() - HEAD) % RECORD_BYTES || (v.size() - HEAD) / RECORD_BYTES != n) return false;
		recs.resize(n);
		for (uint64_t i = 0; i < n; ++i)
		{
			uint32_t w[OV_WORDS];
			for (uint32_t k = 0; k < OV_WORDS; ++k) w[k] = (uint32_t)le(HEAD + i * RECORD_BYTES + 4 * (size_t)k, 4);
			cl_overlap& o = recs[i];
			o.q = w[0]; o.t = w[1]; o.qlen = w[2]; o.tlen = w[3]; o.qs = w[4]; o.qe = w[5]; o.ts = w[6]; o.te = w[7]; o.matches = w[8]; o.subst = w[9]; o.anchor_bases = w[10]; o.flags = w[11];
		}
		return true;
	}
};

// the stored overlaps of an archive: 0 none, 1 read, -1 a `hipoverlaps` stream this build cannot read
inline int read_hipoverlaps(const std::string& path, OverlapSet& out)
{
	ArchiveReader ar;
	if (!ar.open(path)) return 0;
	const int s = ar.id("hipoverlaps");
	std::vector<uint8_t> b; uint64_t meta = 0; int r = 0;
	if (s >= 0) r = ar.part(s, 0, b, meta) && out.unpack(b) ? 1 : -1;
	ar.close();
	return r;
}

// PAF, a line per record whose block length is at least min_block: query, qlen, qs, qe, strand, target, tlen, ts, te, matches, block, 255, then
// mm:i: (subst), an:i: (anchor bases), tp:A:P (the main reference) or tp:A:S (an alternative).  names (or null): the id of every read of the
// input; without them a read's name is its index.  false: a record names a read the names do not hold.
inline bool print_paf(FILE* f, const OverlapSet& S, uint64_t min_block, const std::vector<std::string>* names)
{
	for (const cl_overlap& o : S.recs)
	{
		const uint64_t blk = ov_block(o);
		if (blk < min_block) continue;
		if (names && (o.q >= names->size() || o.t >= names->size())) return false;
		const std::string q = names ? (*names)[o.q] : std::to_string(o.q), t = names ? (*names)[o.t] : std::to_string(o.t);
		fprintf(f, "%s\t%u\t%u\t%u\t%c\t%s\t%u\t%u\t%u\t%u\t%llu\t255\tmm:i:%u\tan:i:%u\ttp:A:%c\n", q.c_str(), o.qlen, o.qs, o.qe, (o.flags & OV_REV) ? '-' : '+', t.c_str(), o.tlen, o.ts, o.te, o.matches,
			(unsigned long long)blk, o.subst, o.anchor_bases, (o.flags & OV_MAIN) ? 'P' : 'S');
	}
	return true;
}
