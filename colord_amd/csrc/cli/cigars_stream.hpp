// cigars_stream.hpp — the `hipcigars` stream of an archive: the base-level CIGAR of every record of the `hipmappings` stream
// (`colord_hip compress-* -G genome.fa --mappings --cigars`), made on the device from the tuple streams, printed by `colord_hip info --mappings
// --cigar` as the PAF of --mappings with cg:Z: appended and by `info --mappings --sam` as SAM, without decoding `dna` or `qual` and without a GPU.
// One part, little-endian:
//   u32 version = 1, u32 operation size = 4, u64 records, u64 operations, then the u32 counts per record, then the operations
// An operation is len << 4 | op with BAM's codes (I 1, D 2, = 7, X 8), in WALK order: the operations of a record taken reversed are reversed here,
// where they are printed.  The reference's decompressor finds its streams by name and never sees this one; `decompress` and `check` ignore it.
// The reader holds every record's operations against its mapping record (cigars.hpp: cg_check) and refuses a stream that breaks one relation.
#pragma once
#include "mappings_stream.hpp"
#include "../cigars.hpp"

struct CigarSet {
	std::vector<uint32_t> rec_ops, ops;                                        // a count per record of the mappings, the operations one behind the other
	std::vector<uint64_t> off;                                                 // unpack: where a record's operations start (records + 1 entries)
	static constexpr uint32_t VERSION = 1;
	static constexpr size_t HEAD = 24;
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
		if (le(0, 4) != VERSION || le(4, 4) != CG_OP_BYTES) return false;
		const uint64_t nr = le(8, 8), no = le(16, 8), words = (v.size() - HEAD) / 4;
		if ((v.size() - HEAD) % 4 || nr > words || no != words - nr || nr != M.recs.size()) return false;      // (nothing is reserved for a count the bytes cannot hold)
		rec_ops.resize(nr); ops.resize(no); off.assign(nr + 1, 0);
		for (uint64_t i = 0; i < nr; ++i) { rec_ops[i] = (uint32_t)le(HEAD + 4 * i, 4); off[i + 1] = off[i] + rec_ops[i]; }
		for (uint64_t i = 0; i < no; ++i) ops[i] = (uint32_t)le(HEAD + 4 * (nr + i), 4);
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
// ... and its header alone, for the line of `colord_hip info`: 0 none, 1 read, -1 the bytes are not a version-1 header
inline int peek_hipcigars(const std::string& path, uint64_t& records, uint64_t& operations)
{
	ArchiveReader ar;
	if (!ar.open(path)) return 0;
	const int s = ar.id("hipcigars");
	std::vector<uint8_t> b; uint64_t meta = 0; int r = 0;
	if (s >= 0)
	{
		auto le = [&](size_t at, int n) { uint64_t x = 0; for (int i = 0; i < n; ++i) x |= (uint64_t)b[at + i] << (8 * i); return x; };
		r = ar.part(s, 0, b, meta) && b.size() >= CigarSet::HEAD && le(0, 4) == CigarSet::VERSION && le(4, 4) == CG_OP_BYTES ? 1 : -1;
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
