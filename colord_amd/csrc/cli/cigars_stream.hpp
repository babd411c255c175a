// cigars_stream.hpp — the `hipcigars` stream of an archive: the base-level CIGAR of every record of the `hipmappings` stream
// (`colord_hip compress-* -G genome.fa --mappings --cigars`), made on the device from the tuple streams, printed by `colord_hip info --mappings
// --cigar` as the PAF of --mappings with cg:Z: appended and by `info --mappings --sam` as SAM, without decoding `dna` or `qual` and without a GPU.
// One part, little-endian:
//   u32 version = 1, u32 operation size = 4, u64 records, u64 operations, then the u32 counts per record, then the operations
// or, written with --cigars-coded, the operations as the segments of ../cigar_coder.hpp, coded on the device:
//   u32 version = 2, u32 operation size = 4, u64 records, u64 operations, u64 segments, u64 segment bytes, the u32 counts per record, the segments
// Both versions are read into the same CigarSet; a version-2 stream is decoded first (cgc_unpack refuses what is no whole segments of its format),
// then every check below runs as for version 1.
// An operation is len << 4 | op with BAM's codes (I 1, D 2, = 7, X 8), in WALK order: the operations of a record taken reversed are reversed here,
// where they are printed.  The reference's decompressor finds its streams by name and never sees this one; `decompress` and `check` ignore it.
// The reader holds every record's operations against its mapping record (cigars.hpp: cg_check) and refuses a stream that breaks one relation.
#pragma once
#include "mappings_stream.hpp"
#include "../cigars.hpp"
#include "../cigar_coder.hpp"

struct CigarSet {
	std::vector<uint32_t> rec_ops, ops;                                        // a count per record of the mappings, the operations one behind the other
	std::vector<uint64_t> off;                                                 // unpack: where a record's operations start (records + 1 entries)
	static constexpr uint32_t VERSION = 1;
	static constexpr size_t HEAD = 24;
	static constexpr uint32_t VERSION_CODED = 2;
	static constexpr size_t HEAD_CODED = 40;
	uint32_t version = VERSION;                                                // unpack: the version that was read
	uint64_t coded_bytes = 0, coded_segments = 0, coded_escapes = 0;           // ... and of a version-2 stream, its segments
	// version 2: the counts and the coded segments of n_ops operations
	static std::vector<uint8_t> pack_coded(const std::vector<uint32_t>& rec_ops, const std::vector<uint8_t>& segments, uint64_t n_ops, uint64_t n_segments)
	{
		std::vector<uint8_t> v; v.reserve(HEAD_CODED + rec_ops.size() * 4 + segments.size());
		auto le = [&](uint64_t x, int n) { for (int i = 0; i < n; ++i) v.push_back((uint8_t)(x >> (8 * i))); };
		le(VERSION_CODED, 4); le(CG_OP_BYTES, 4); le(rec_ops.size(), 8); le(n_ops, 8); le(n_segments, 8); le(segments.size(), 8);
		for (uint32_t c : rec_ops) le(c, 4);
		v.insert(v.end(), segments.begin(), segments.end());
		return v;
	}
	std::vector<uint8_t> pack() const
	{
		std::vector<uint8_t> v; v.reserve(HEAD + (rec_ops.size() + ops.size()) * 4);
		auto le = [&](uint64_t x, int n) { for (int i = 0; i < n; ++i) v.push_back((uint8_t)(x >> (8 * i))); };
		le(VERSION, 4); le(CG_OP_BYTES, 4); le(rec_ops.size(), 8); le(ops.size(), 8);
		for (uint32_t c : rec_ops) le(c, 4);
		for (uint32_t w : ops) le(w, 4);
		return v;
	}
	// false: another version or operation size, sizes the bytes do not hold, a record count that is not the mappings', counts that do not add up
	// to the operations, a record whose operations break a relation against its mapping record
	bool unpack(const std::vector<uint8_t>& v, const MappingSet& M)
	{
		rec_ops.clear(); ops.clear(); off.clear();
		if (v.size() < HEAD) return false;
		auto le = [&](size_t at, int n) { uint64_t x = 0; for (int i = 0; i < n; ++i) x |= (uint64_t)v[at + i] << (8 * i); return x; };
		version = (uint32_t)le(0, 4); coded_bytes = coded_segments = coded_escapes = 0;
		if ((version != VERSION && version != VERSION_CODED) || le(4, 4) != CG_OP_BYTES) return false;
		const uint64_t nr = le(8, 8), no = le(16, 8);
		if (version == VERSION_CODED)
		{	// the sizes against the bytes, the segments decoded, their counts against the header
			if (v.size() < HEAD_CODED) return false;
			const uint64_t ns = le(24, 8), nb = le(32, 8), rest = v.size() - HEAD_CODED;
			if (nr > rest / 4 || nb != rest - 4 * nr || nr != M.recs.size() || no > nb * (uint64_t)CGC_SEG_OPS) return false;      // (nothing is reserved for a count the bytes cannot hold)
			uint64_t got_seg = 0, got_esc = 0;
			if (cgc_unpack(v.data() + HEAD_CODED + 4 * nr, nb, ops, &got_seg, &got_esc) != CGC_OK || ops.size() != no || got_seg != ns) { ops.clear(); return false; }
			coded_bytes = nb; coded_segments = ns; coded_escapes = got_esc;
			rec_ops.resize(nr); off.assign(nr + 1, 0);
			for (uint64_t i = 0; i < nr; ++i) { rec_ops[i] = (uint32_t)le(HEAD_CODED + 4 * i, 4); off[i + 1] = off[i] + rec_ops[i]; }
		}
		else
		{
			const uint64_t words = (v.size() - HEAD) / 4;
			if ((v.size() - HEAD) % 4 || nr > words || no != words - nr || nr != M.recs.size()) return false;      // (nothing is reserved for a count the bytes cannot hold)
			rec_ops.resize(nr); ops.resize(no); off.assign(nr + 1, 0);
			for (uint64_t i = 0; i < nr; ++i) { rec_ops[i] = (uint32_t)le(HEAD + 4 * i, 4); off[i + 1] = off[i] + rec_ops[i]; }
			for (uint64_t i = 0; i < no; ++i) ops[i] = (uint32_t)le(HEAD + 4 * (nr + i), 4);
		}
		bool ok = off[nr] == no;
		for (uint64_t i = 0; ok && i < nr; ++i) ok = M.recs[i].qe <= M.recs[i].qlen && cg_check(M.recs[i], ops.data() + off[i], rec_ops[i]) == 0;      // (qe <= qlen: the hard clips of SAM)
		if (!ok) { rec_ops.clear(); ops.clear(); off.clear(); }
		return ok;
	}
	// the operations of record i as CIGAR text, the target forward: reversed for a record taken reversed
	std::string text(uint64_t i, bool rev) const
	{
		std::string s;
		const uint64_t a = off[i], n = rec_ops[i];
		for (uint64_t k = 0; k < n; ++k) { const uint32_t w = ops[a + (rev ? n - 1 - k : k)]; s += std::to_string(cg_len(w)); s += cg_char(cg_op(w)); }
		return s;
	}
	// NM: the bases of X, I and D
	uint64_t edit_distance(uint64_t i) const
	{
		uint64_t nm = 0;
		for (uint64_t k = off[i]; k < off[i + 1]; ++k) if (cg_op(ops[k]) != CG_EQ) nm += cg_len(ops[k]);
		return nm;
	}
};

// the stored CIGARs of an archive against its mappings M: 0 none, 1 read, -1 a `hipcigars` stream this build cannot read
inline int read_hipcigars(const std::string& path, const MappingSet& M, CigarSet& out)
{
	ArchiveReader ar;
	if (!ar.open(path)) return 0;
	const int s = ar.id("hipcigars");
	std::vector<uint8_t> b; uint64_t meta = 0; int r = 0;
	if (s >= 0) r = ar.part(s, 0, b, meta) && out.unpack(b, M) ? 1 : -1;
	ar.close();
	return r;
}
// ... and its header alone, for the line of `colord_hip info`: 0 none, 1 read, -1 the bytes are not a header of version 1 or 2 (of version 2: with
// segment headers that fit the bytes and add up to the operations; *coded takes what they say)
struct CigarCoded { uint32_t version = 0; uint64_t bytes = 0, segments = 0, escapes = 0; };
inline int peek_hipcigars(const std::string& path, uint64_t& records, uint64_t& operations, CigarCoded* coded = nullptr)
{
	ArchiveReader ar;
	if (!ar.open(path)) return 0;
	const int s = ar.id("hipcigars");
	std::vector<uint8_t> b; uint64_t meta = 0; int r = 0;
	if (s >= 0)
	{
		auto le = [&](size_t at, int n) { uint64_t x = 0; for (int i = 0; i < n; ++i) x |= (uint64_t)b[at + i] << (8 * i); return x; };
		r = ar.part(s, 0, b, meta) && b.size() >= CigarSet::HEAD && (le(0, 4) == CigarSet::VERSION || le(0, 4) == CigarSet::VERSION_CODED) && le(4, 4) == CG_OP_BYTES ? 1 : -1;
		if (r > 0 && le(0, 4) == CigarSet::VERSION_CODED)
		{
			CigarCoded c; c.version = 2;
			uint64_t no = 0;
			const uint64_t nr = b.size() >= CigarSet::HEAD_CODED ? le(8, 8) : 0, rest = b.size() >= CigarSet::HEAD_CODED ? b.size() - CigarSet::HEAD_CODED : 0;
			if (b.size() < CigarSet::HEAD_CODED || nr > rest / 4 || le(32, 8) != rest - 4 * nr) r = -1;
			else
			{
				c.bytes = le(32, 8);
				if (cgc_scan(b.data() + CigarSet::HEAD_CODED + 4 * nr, c.bytes, &no, &c.segments, &c.escapes) != CGC_OK || no != le(16, 8) || c.segments != le(24, 8)) r = -1;
			}
			if (r > 0 && coded) *coded = c;
		}
		else if (r > 0 && coded) coded->version = 1;
		if (r > 0) { records = le(8, 8); operations = le(16, 8); }
	}
	ar.close();
	return r;
}

// The PAF of print_mappings_paf with cg:Z: appended.  A record hidden by min_block takes its CIGAR with it.
inline bool print_mappings_paf_cigar(FILE* f, const MappingSet& S, const CigarSet& G, uint64_t min_block, const std::vector<std::string>* names)
{
	for (size_t i = 0; i < S.recs.size(); ++i)
	{
		const cl_overlap& o = S.recs[i];
		const uint64_t blk = ov_block(o);
		if (blk < min_block) continue;
		if (names && o.q >= names->size()) return false;
		const std::string q = names ? (*names)[o.q] : std::to_string(o.q);
		fprintf(f, "%s\t%u\t%u\t%u\t%c\t%s\t%llu\t%u\t%u\t%u\t%llu\t255\tmm:i:%u\tan:i:%u\ttp:A:%c\tcg:Z:%s\n", q.c_str(), o.qlen, o.qs, o.qe, (o.flags & OV_REV) ? '-' : '+', S.name_of(o.t).c_str(),
			(unsigned long long)S.seq_len[o.t], o.ts, o.te, o.matches, (unsigned long long)blk, o.subst, o.anchor_bases, (o.flags & OV_MAIN) ? 'P' : 'S', G.text(i, (o.flags & OV_REV) != 0).c_str());
	}
	return true;
}

// SAM: @HD, @SQ from the sequence table, then a line per record: QNAME (the read's index, or its name), FLAG 0 / 16 plus 2048 on every record
// of a read but its first, RNAME, POS ts + 1, MAPQ 255, the CIGAR with hard clips for the unaligned read ends (swapped for a record taken
// reversed: SAM has the read reverse-complemented there), * 0 0 * *, NM:i: = the bases of X, I and D.
inline bool print_mappings_sam(FILE* f, const MappingSet& S, const CigarSet& G, uint64_t min_block, const std::vector<std::string>* names)
{
	fprintf(f, "@HD\tVN:1.6\tSO:unknown\n");
	for (size_t s = 0; s < S.seq_len.size(); ++s) fprintf(f, "@SQ\tSN:%s\tLN:%llu\n", S.name_of((uint32_t)s).c_str(), (unsigned long long)S.seq_len[s]);
	for (size_t i = 0; i < S.recs.size(); ++i)
	{
		const cl_overlap& o = S.recs[i];
		const bool rev = (o.flags & OV_REV) != 0, later = i && S.recs[i - 1].q == o.q;      // (the records of a read follow each other)
		if (ov_block(o) < min_block) continue;
		if (names && o.q >= names->size()) return false;
		const std::string q = names ? (*names)[o.q] : std::to_string(o.q);
		const uint32_t head = rev ? o.qlen - o.qe : o.qs, tail = rev ? o.qs : o.qlen - o.qe;
		std::string cg = G.text(i, rev);
		if (head) cg = std::to_string(head) + "H" + cg;
		if (tail) cg += std::to_string(tail) + "H";
		fprintf(f, "%s\t%u\t%s\t%u\t255\t%s\t*\t0\t0\t*\t*\tNM:i:%llu\n", q.c_str(), (rev ? 16u : 0u) | (later ? 2048u : 0u), S.name_of(o.t).c_str(), o.ts + 1, cg.c_str(), (unsigned long long)G.edit_distance(i));
	}
	return true;
}
