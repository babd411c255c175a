// cigar_coder.hpp — the coded form of CIGAR operations: the words len << 4 | op of cigars.hpp as the bytes of a static-model
// interval coder.  The definition, once — symbols, contexts, bins, segment bytes — shared by the kernels (cigar_coder.hip), the host twin and
// the reader (cli/cigars_stream.hpp).
//
// SYMBOLS.  A word gives two: the op symbol o (I 0, D 1, = 2, X 3) and the length symbol l = len - 1 for len <= 255, else 255 (ESCAPE); an
// escaped operation appends its len as a raw u32 to its segment's escape list, in operation order.  The coder takes ANY sequence of words with
// a valid op and len >= 1 (equal neighbours occur across record boundaries); anything else is refused with the index of the first such word.
// CONTEXTS.  o is coded in the context of the o of the operation before it in flat order, the first operation of a part in context 4: five rows
// of 4 symbols.  l is coded in the context of its own o: four rows of 256 symbols.  Record boundaries play no role.
// SEGMENTS, PARTS.  The operations of a call are cut into segments of seg_ops (default and maximum 2^20), a segment into parts of part_ops
// (default 4096; the packers take up to 2^16, the reader any); the last of either is shorter.  A part is one restart of the coder (low 0, range
// MASK, 8 bytes of low at its end, exactly k_range_code's): its symbols are 2 j and 2 j + 1 for its j-th operation.
// MODEL.  Static per segment: the 20 + 1024 counts of the segment's symbols ARE the frequencies, cum the sum of the counts of the lower symbols
// of the row, tot the row's sum — at most 2^20 operations keep every tot below 2^21, nothing is rescaled and nothing adapts.  A triple depends on
// its own operation, the operation before it and the table: the model stage is a lane per operation without a chain, the decoder a table search.
// SEGMENT BYTES (little-endian): u32 n_ops, u32 part_ops, u32 n_escapes, u32 table_bytes; the ceil(n_ops / part_ops) part sizes as u32; the 1044
// counts as LEB128, op rows first, row-major; the escapes as u32; the parts one behind the other.
//
// Under a host compiler alone this header needs no HIP (tests/tools/cigarcoder_host_test.cpp).
#pragma once
#include <algorithm>
#include "cigars.hpp"
#include "host_coder.hpp"

constexpr uint32_t CGC_SEG_OPS = 1u << 20, CGC_PART_OPS = 4096, CGC_PART_OPS_MAX = 1u << 16;
constexpr uint32_t CGC_OP_ROWS = 5, CGC_OP_BINS = 20, CGC_LEN_SYMS = 256, CGC_BINS = CGC_OP_BINS + 4 * CGC_LEN_SYMS, CGC_ROWS = 9, CGC_ESC = 255;
constexpr uint32_t CGC_HEAD = 16;
// why a segment is refused (cl_cigars_check_host; cgc_refusal_text)
enum : uint32_t { CGC_OK = 0, CGC_R_SIZES = 1, CGC_R_HEADER = 2, CGC_R_TABLE = 3, CGC_R_TABLE_SUM = 4, CGC_R_TOT0 = 5, CGC_R_SYMBOL = 6, CGC_R_ESCAPES = 7, CGC_R_ESC_VALUE = 8, CGC_R_PART_END = 9 };
inline const char* cgc_refusal_text(uint32_t r)
{
	static const char* const T[] = { "ok", "sizes the bytes do not hold", "a segment header out of range", "a malformed count table", "a table that does not sum to the symbols",
		"a context in use has the total 0", "a decoded symbol with the count 0", "escapes run out or are left over", "an escape below 256 or past the longest run", "a part does not end at its size" };
	return r < sizeof(T) / sizeof(T[0]) ? T[r] : "unknown";
}

ED_HD inline uint32_t cgc_op_index(uint32_t op) { return op == CG_I ? 0u : op == CG_D ? 1u : op == CG_EQ ? 2u : op == CG_X ? 3u : 4u; }      // 4: no operation of a CIGAR here
ED_HD inline uint32_t cgc_op_code(uint32_t o) { return o == 0 ? CG_I : o == 1 ? CG_D : o == 2 ? CG_EQ : CG_X; }
ED_HD inline bool cgc_valid(uint32_t w) { return cgc_op_index(cg_op(w)) < 4 && cg_len(w) >= 1; }
ED_HD inline uint32_t cgc_len_sym(uint32_t len) { return len <= 255 ? len - 1 : CGC_ESC; }
ED_HD inline uint32_t cgc_op_bin(uint32_t row, uint32_t o) { return row * 4 + o; }                // row: the o before, 4 at a part's first operation
ED_HD inline uint32_t cgc_len_bin(uint32_t o, uint32_t l) { return CGC_OP_BINS + o * CGC_LEN_SYMS + l; }
ED_HD inline uint32_t cgc_row_first(uint32_t row) { return row < CGC_OP_ROWS ? row * 4 : CGC_OP_BINS + (row - CGC_OP_ROWS) * CGC_LEN_SYMS; }
ED_HD inline uint32_t cgc_row_syms(uint32_t row) { return row < CGC_OP_ROWS ? 4u : CGC_LEN_SYMS; }
// the knobs of a packer: 0 is the default; false: out of range
ED_HD inline bool cgc_knobs(uint32_t& part_ops, uint32_t& seg_ops)
{
	if (!part_ops) part_ops = CGC_PART_OPS;
	if (!seg_ops) seg_ops = CGC_SEG_OPS;
	return part_ops <= CGC_PART_OPS_MAX && seg_ops <= CGC_SEG_OPS;
}

// the rows of a segment's table, cumulative
struct CgcModel {
	uint32_t freq[CGC_BINS], cum[CGC_BINS], tot[CGC_ROWS];
	void build(const uint32_t* counts)
	{
		for (uint32_t r = 0; r < CGC_ROWS; ++r)
		{
			uint32_t t = 0;
			for (uint32_t b = cgc_row_first(r), e = b + cgc_row_syms(r); b < e; ++b) { freq[b] = counts[b]; cum[b] = t; t += counts[b]; }
			tot[r] = t;
		}
	}
};

// The host's encoder: the interval arithmetic of k_range_code (rc_dev.hpp), a symbol at a time.
struct CgcRangeEnc {
	static constexpr uint64_t TOP = 0x00ffffffffffffULL, MASK = 0xff00000000000000ULL;
	uint64_t low = 0, range = MASK;
	std::vector<uint8_t>& out;
	explicit CgcRangeEnc(std::vector<uint8_t>& o) : out(o) {}
	void encode(uint32_t cum, uint32_t freq, uint32_t tot)
	{
		const uint64_t q = range / tot;
		low += q * cum; range = q * freq;
		while (range <= TOP)
		{
			if ((low ^ (low + range)) & MASK) range = (low | TOP) - low;
			out.push_back((uint8_t)(low >> 56));
			low <<= 8; range <<= 8;
		}
	}
	void end() { for (int i = 0; i < 8; ++i) { out.push_back((uint8_t)(low >> 56)); low <<= 8; } }
};

inline void cgc_le32(std::vector<uint8_t>& v, uint32_t x) { for (int i = 0; i < 4; ++i) v.push_back((uint8_t)(x >> (8 * i))); }
// A segment's bytes appended to out, from its pieces (the host twin's, or the device's copied over).
inline void cgc_segment_bytes(std::vector<uint8_t>& out, uint32_t n_ops, uint32_t part_ops, const uint32_t* counts, const uint32_t* escapes, uint32_t n_escapes, const uint32_t* part_sizes, uint32_t n_parts,
                              const uint8_t* parts, uint64_t parts_bytes)
{
	std::vector<uint8_t> table;
	for (uint32_t b = 0; b < CGC_BINS; ++b) { uint32_t x = counts[b]; do { table.push_back((uint8_t)((x & 0x7f) | (x > 0x7f ? 0x80 : 0))); x >>= 7; } while (x); }
	cgc_le32(out, n_ops); cgc_le32(out, part_ops); cgc_le32(out, n_escapes); cgc_le32(out, (uint32_t)table.size());
	for (uint32_t p = 0; p < n_parts; ++p) cgc_le32(out, part_sizes[p]);
	out.insert(out.end(), table.begin(), table.end());
	for (uint32_t e = 0; e < n_escapes; ++e) cgc_le32(out, escapes[e]);
	out.insert(out.end(), parts, parts + parts_bytes);
}

// The host twin: the segments of n words appended to out, on one thread.  false: a knob out of range (*bad = ~0) or a word that is no
// operation (*bad = the first such index); out is unchanged then.
inline bool cgc_pack_host(const uint32_t* ops, uint64_t n, uint32_t part_ops, uint32_t seg_ops, std::vector<uint8_t>& out, uint64_t* bad, uint64_t* n_escapes = nullptr)
{
	if (bad) *bad = ~0ull;
	if (!cgc_knobs(part_ops, seg_ops)) return false;
	for (uint64_t i = 0; i < n; ++i) if (!cgc_valid(ops[i])) { if (bad) *bad = i; return false; }
	uint64_t esc_total = 0;
	std::vector<uint32_t> counts(CGC_BINS), escapes, sizes; std::vector<uint8_t> parts;
	CgcModel M;
	for (uint64_t s0 = 0; s0 < n; s0 += seg_ops)
	{
		const uint32_t sn = (uint32_t)std::min<uint64_t>(seg_ops, n - s0);
		const uint32_t* w = ops + s0;
		std::fill(counts.begin(), counts.end(), 0u); escapes.clear(); sizes.clear(); parts.clear();
		for (uint32_t i = 0; i < sn; ++i)
		{
			const uint32_t o = cgc_op_index(cg_op(w[i])), row = i % part_ops ? cgc_op_index(cg_op(w[i - 1])) : 4u, l = cgc_len_sym(cg_len(w[i]));
			++counts[cgc_op_bin(row, o)]; ++counts[cgc_len_bin(o, l)];
			if (l == CGC_ESC) escapes.push_back(cg_len(w[i]));
		}
		M.build(counts.data());
		for (uint32_t p0 = 0; p0 < sn; p0 += part_ops)
		{
			const size_t before = parts.size();
			CgcRangeEnc E(parts);
			uint32_t row = 4;
			for (uint32_t i = p0, e = std::min(sn, p0 + part_ops); i < e; ++i)
			{
				const uint32_t o = cgc_op_index(cg_op(w[i])), ob = cgc_op_bin(row, o), lb = cgc_len_bin(o, cgc_len_sym(cg_len(w[i])));
				E.encode(M.cum[ob], M.freq[ob], M.tot[row]);
				E.encode(M.cum[lb], M.freq[lb], M.tot[CGC_OP_ROWS + o]);
				row = o;
			}
			E.end();
			sizes.push_back((uint32_t)(parts.size() - before));
		}
		cgc_segment_bytes(out, sn, part_ops, counts.data(), escapes.data(), (uint32_t)escapes.size(), sizes.data(), (uint32_t)sizes.size(), parts.data(), parts.size());
		esc_total += escapes.size();
	}
	if (n_escapes) *n_escapes = esc_total;
	return true;
}

// What a segment's header says: its sizes, held against the n bytes at b.  CGC_OK: *used = the segment's bytes.
struct CgcSegment { uint32_t n_ops, part_ops, n_escapes, table_bytes, n_parts; uint64_t sizes_at, table_at, esc_at, parts_at, used; };
inline uint32_t cgc_le32_at(const uint8_t* b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; }
inline uint32_t cgc_segment_head(const uint8_t* b, uint64_t n, CgcSegment& S)
{
	if (n < CGC_HEAD) return CGC_R_SIZES;
	S.n_ops = cgc_le32_at(b); S.part_ops = cgc_le32_at(b + 4); S.n_escapes = cgc_le32_at(b + 8); S.table_bytes = cgc_le32_at(b + 12);
	if (!S.n_ops || S.n_ops > CGC_SEG_OPS || !S.part_ops || S.n_escapes > S.n_ops) return CGC_R_HEADER;
	S.n_parts = (uint32_t)(((uint64_t)S.n_ops + S.part_ops - 1) / S.part_ops);
	S.sizes_at = CGC_HEAD; S.table_at = S.sizes_at + 4ull * S.n_parts; S.esc_at = S.table_at + S.table_bytes; S.parts_at = S.esc_at + 4ull * S.n_escapes;
	if (S.parts_at > n) return CGC_R_SIZES;
	uint64_t sum = 0;
	for (uint32_t p = 0; p < S.n_parts; ++p) sum += cgc_le32_at(b + S.sizes_at + 4ull * p);      // (at most 2^20 sizes below 2^32: no overflow)
	if (sum > n - S.parts_at) return CGC_R_SIZES;
	S.used = S.parts_at + sum;
	return CGC_OK;
}
// The headers alone: the operations, segments and escapes of the n bytes at b.
inline uint32_t cgc_scan(const uint8_t* b, uint64_t n, uint64_t* n_ops, uint64_t* n_seg, uint64_t* n_esc)
{
	uint64_t at = 0, no = 0, ns = 0, ne = 0;
	while (at < n)
	{
		CgcSegment S;
		if (const uint32_t r = cgc_segment_head(b + at, n - at, S)) return r;
		at += S.used; no += S.n_ops; ne += S.n_escapes; ++ns;
	}
	if (n_ops) *n_ops = no;
	if (n_seg) *n_seg = ns;
	if (n_esc) *n_esc = ne;
	return CGC_OK;
}
// One segment decoded, its words appended to ops.  Reads nothing outside [b, b + n).
inline uint32_t cgc_unpack_segment(const uint8_t* b, uint64_t n, uint64_t& used, std::vector<uint32_t>& ops)
{
	CgcSegment S;
	if (const uint32_t r = cgc_segment_head(b, n, S)) return r;
	std::vector<uint32_t> counts(CGC_BINS);
	{	// the table: exactly 1044 values in exactly table_bytes
		uint64_t at = S.table_at; const uint64_t end = S.esc_at;
		for (uint32_t k = 0; k < CGC_BINS; ++k)
		{
			uint32_t x = 0; int shift = 0;
			for (;;)
			{
				if (at >= end || shift > 21) return CGC_R_TABLE;
				const uint8_t c = b[at++];
				x |= (uint32_t)(c & 0x7f) << shift; shift += 7;
				if (!(c & 0x80)) break;
			}
			if (x > S.n_ops) return CGC_R_TABLE_SUM;
			counts[k] = x;
		}
		if (at != end) return CGC_R_TABLE;
	}
	CgcModel M; M.build(counts.data());
	{	// the rows against the symbols: every operation has an op symbol, a part's first in row 4, and a length symbol in the row of its op
		uint64_t all = 0, esc = 0;
		for (uint32_t r = 0; r < CGC_OP_ROWS; ++r) all += M.tot[r];
		if (all != S.n_ops || M.tot[4] != S.n_parts) return CGC_R_TABLE_SUM;
		for (uint32_t o = 0; o < 4; ++o)
		{
			uint64_t with = 0;
			for (uint32_t r = 0; r < CGC_OP_ROWS; ++r) with += counts[cgc_op_bin(r, o)];
			if (with != M.tot[CGC_OP_ROWS + o]) return CGC_R_TABLE_SUM;
			esc += counts[cgc_len_bin(o, CGC_ESC)];
		}
		if (esc != S.n_escapes) return CGC_R_ESCAPES;
	}
	const size_t before = ops.size();
	auto fail = [&](uint32_t r) { ops.resize(before); return r; };
	uint64_t part_at = S.parts_at; uint32_t esc_used = 0;
	for (uint32_t p = 0; p < S.n_parts; ++p)
	{
		const uint32_t size = cgc_le32_at(b + S.sizes_at + 4ull * p);
		const uint32_t len = (uint32_t)std::min<uint64_t>(S.part_ops, S.n_ops - (uint64_t)p * S.part_ops);
		if (size < 8) return fail(CGC_R_PART_END);
		hostrc::RangeDec rc; rc.start(b + part_at, size);
		uint32_t row = 4;
		for (uint32_t i = 0; i < len; ++i)
		{
			uint32_t sym[2];
			for (int half = 0; half < 2; ++half)
			{
				const uint32_t r = half ? CGC_OP_ROWS + sym[0] : row, tot = M.tot[r];
				if (!tot) return fail(CGC_R_TOT0);
				rc.scale(tot);                                                       // the target buffer / range is only compared (host_coder.hpp): products, no second division
				if (rc.below(tot)) return fail(CGC_R_SYMBOL);
				uint32_t k = cgc_row_first(r);
				while (rc.below((uint64_t)M.cum[k] + M.freq[k])) ++k;                // (target < tot: the search ends inside the row, at a count that is not 0)
				rc.update(M.freq[k], M.cum[k]);
				sym[half] = k - cgc_row_first(r);
			}
			uint32_t lenv = sym[1] + 1;
			if (sym[1] == CGC_ESC)
			{
				if (esc_used == S.n_escapes) return fail(CGC_R_ESCAPES);
				lenv = cgc_le32_at(b + S.esc_at + 4ull * esc_used++);
				if (lenv < 256 || lenv > CG_LEN_MAX) return fail(CGC_R_ESC_VALUE);
			}
			ops.push_back(lenv << 4 | cgc_op_code(sym[0]));
			row = sym[0];
		}
		if (rc.over || rc.pos != size) return fail(CGC_R_PART_END);
		part_at += size;
	}
	if (esc_used != S.n_escapes) return fail(CGC_R_ESCAPES);
	used = S.used;
	return CGC_OK;
}
// All segments of the n bytes at b, their words appended to ops (unchanged when refused).
inline uint32_t cgc_unpack(const uint8_t* b, uint64_t n, std::vector<uint32_t>& ops, uint64_t* n_seg = nullptr, uint64_t* n_esc = nullptr)
{
	const size_t before = ops.size();
	uint64_t no = 0, ns = 0, ne = 0;
	if (const uint32_t r = cgc_scan(b, n, &no, &ns, &ne)) return r;
	ops.reserve(before + no);
	for (uint64_t at = 0; at < n;)
	{
		uint64_t used = 0;
		if (const uint32_t r = cgc_unpack_segment(b + at, n - at, used, ops)) { ops.resize(before); return r; }
		at += used;
	}
	if (n_seg) *n_seg = ns;
	if (n_esc) *n_esc = ne;
	return CGC_OK;
}
