// pileup.hpp — per-position base counts of a reference-genome run.  With -G every read is aligned base by base against
// pieces of the genome (the pseudo reads, reference ids 0 .. n_pseudo-1; mappings.hpp has their geometry); the pileup keeps, for every
// position of the genome, what the reads said there.  On the device: k_pileup_walk, k_pileup_fold, k_pileup_sites (pileup.hip).  Here:
// the table's layout, where a tuple lands — ONE function for the kernel and the host twin, so that the two cannot disagree — the site
// decision with the record's layout, ONE function in the same way, and the host twin, a visitor of es_walk_host (es_codes.hpp) that
// owns no check of its own.
//
// Table: n_pos = sum of seq_len[s] positions, sequence s from seq_base[s] on; per position PU_COLS 32-bit counters (they wrap at 2^32):
//   match (match tuples and anchor bases), sub[A C G T] (substitutions by the READ's base in the genome's forward orientation), del (one
//   per deleted reference base), ins (one per insertion RUN, at the forward position left of it), ref (the genome's base, filled at finish).
// Anchors are booked as a difference, diff[a] += 1 and diff[a + L] -= 1 modulo 2^32 over n_pos + 1 entries; the fold adds the running
// sum of diff to `match`.  Tuples met on a reference id >= n_pseudo (a read) count nothing.
//
// An insertion run is a maximal row of consecutive ins tuples in the stream; it counts ONCE, at the forward position left of it: taken
// forward that is cursor - 1 (none at cursor 0, and none when skips have taken the cursor past the piece's end), taken reversed
// len - 1 - cursor (none at cursor >= len).  A run without such a position is counted in ins_unplaced alone.
//
// Under a host compiler alone this header needs no HIP (tests/tools/pileup_host_test.cpp).
#pragma once
#include <vector>
#include "mappings.hpp"

constexpr uint32_t PU_COLS = 8;
enum : uint32_t { PU_MATCH = 0, PU_SUB = 1, PU_DEL = 5, PU_INS = 6, PU_REF = 7 };
constexpr uint32_t PU_KIND_DEL = 4, PU_KIND_INS = 5;                        // a site's kind: 0..3 a base, then these
constexpr uint32_t PU_SITE_WORDS = 12, PU_SUMS = 7;
static_assert(sizeof(cl_pileup_site) == PU_SITE_WORDS * 4, "cl_pileup_site is twelve 32-bit words without padding");
static_assert(sizeof(cl_pileup_sums) == PU_SUMS * 8, "cl_pileup_sums is seven 64-bit words without padding");
enum : uint32_t { PU_S_COVERED = 0, PU_S_MATCH, PU_S_SUB, PU_S_DEL, PU_S_INS, PU_S_UNPLACED, PU_S_READS };
constexpr uint32_t PU_TILE = 512;                                           // positions a wave folds or searches for sites in one go (8 rounds of 64)

// seq_base: n_seqs + 1 entries, seq_base[n_seqs] = n_pos; piece_first: n_seqs + 1 entries (mappings.hpp); origin: the table position of
// the first base of every piece, n_pseudo entries (host or device pointers, as the caller runs)
struct PileGeom { const uint64_t* seq_base; const uint32_t* piece_first; const uint32_t* origin; uint64_t n_pos; uint32_t n_seqs, n_pseudo, read_len, step; };
struct PileThresholds { uint32_t min_depth, min_alt, min_permille; };

// The tables of a geometry.  The refusals of map_piece_first, and CL_E_UNSUPPORTED for a table of 2^32 positions or more.
inline cl_status pile_geometry(const uint64_t* seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap, std::vector<uint32_t>& piece_first, std::vector<uint64_t>& seq_base,
                               std::vector<uint32_t>& origin)
{
	seq_base.assign((size_t)n_seqs + 1, 0); origin.clear();
	const cl_status s = map_piece_first(seq_len, n_seqs, read_len, overlap, piece_first);
	if (s != CL_OK) return s;
	for (uint32_t i = 0; i < n_seqs; ++i) { seq_base[i + 1] = seq_base[i] + seq_len[i]; if (seq_base[i + 1] > OV_POS_MAX) return CL_E_UNSUPPORTED; }
	origin.resize(piece_first[n_seqs]);
	const uint64_t step = read_len - overlap;
	for (uint32_t i = 0; i < n_seqs; ++i)
		for (uint32_t p = piece_first[i]; p < piece_first[i + 1]; ++p) origin[p] = (uint32_t)(seq_base[i] + (uint64_t)(p - piece_first[i]) * step);
	return CL_OK;
}
// the length the geometry gives piece p of sequence s
inline uint64_t pile_piece_len(const uint64_t* seq_len, const std::vector<uint32_t>& piece_first, uint32_t s, uint32_t p, uint32_t read_len, uint32_t overlap)
{
	const uint64_t start = (uint64_t)(p - piece_first[s]) * (read_len - overlap), rest = seq_len[s] - start;
	return rest < read_len ? rest : read_len;
}

// WHERE A TUPLE LANDS.  The table position of cursor c < len of a piece of len bases that starts at `origin`, taken reversed or not.
ED_HD inline uint64_t pile_at(uint64_t origin, uint32_t len, bool rev, uint64_t c) { return origin + (rev ? (uint64_t)len - 1 - c : c); }
// ... the first position a of an anchor of L > 0 bases at cursor c, c + L <= len: it covers the forward interval [a, a + L)
ED_HD inline uint64_t pile_anchor_start(uint64_t origin, uint32_t len, bool rev, uint64_t c, uint32_t L) { return pile_at(origin, len, rev, rev ? c + L - 1 : c); }
// ... the forward position left of an insertion run met at cursor c; false: there is none
ED_HD inline bool pile_ins_left(uint64_t origin, uint32_t len, bool rev, uint64_t c, uint64_t& pos)
{
	if (rev ? c >= len : (c == 0 || c > len)) return false;
	pos = pile_at(origin, len, rev, rev ? c : c - 1);
	return true;
}
// the READ's base of a subst tuple of value v < 3 on the reference base rb < 4 (as edits.hpp counts it), in the genome's forward orientation
ED_HD inline uint32_t pile_sub_base(uint32_t rb, uint32_t v, bool rev) { const uint32_t b = v + (v >= rb ? 1u : 0u); return rev ? 3u - b : b; }

// the sequence of table position x < n_pos: the first s with seq_base[s + 1] > x (it exists: seq_base[n_seqs] = n_pos), at most 32 steps
// inside seq_base[1 .. n_seqs]
ED_HD inline uint32_t pile_seq_of(const uint64_t* seq_base, uint32_t n_seqs, uint64_t x)
{
	uint32_t lo = 0, hi = n_seqs - 1;
	for (uint32_t it = 0; it < 32 && lo < hi; ++it)
	{
		const uint32_t mid = lo + (hi - lo) / 2;
		if (seq_base[mid + 1] > x) hi = mid; else lo = mid + 1;
	}
	return lo;
}
// the piece that gives position x of the table its reference base, and the offset in it: piece min(xs / step, pieces - 1) of the sequence,
// xs the position in the sequence (xs < pieces * step, and a piece that has a successor is longer than a step: the offset lies in it)
ED_HD inline void pile_ref_place(const PileGeom& G, uint64_t x, uint32_t& id, uint32_t& off)
{
	const uint32_t s = pile_seq_of(G.seq_base, G.n_seqs, x);
	const uint64_t xs = x - G.seq_base[s];
	const uint32_t pieces = G.piece_first[s + 1] - G.piece_first[s];
	uint64_t k = xs / G.step;
	if (k > pieces - 1) k = pieces - 1;
	id = G.piece_first[s] + (uint32_t)k; off = (uint32_t)(xs - k * G.step);
}

// THE SITE DECISION AND THE RECORD.  col: the PU_COLS counters of table position x, folded.  depth = match + sub + del; the ALT is the
// largest of sub[b] for b != ref, del and ins, ties to the lowest kind.  A site: depth >= min_depth, alt >= min_alt and
// alt * 1000 >= min_permille * depth.  The sequence is searched only for a site.
ED_HD inline bool pile_site(const PileGeom& G, uint64_t x, const uint32_t* col, const PileThresholds& T, cl_pileup_site& o)
{
	const uint32_t ref = col[PU_REF] & 3u;
	const uint64_t depth = (uint64_t)col[PU_MATCH] + col[PU_SUB] + col[PU_SUB + 1] + col[PU_SUB + 2] + col[PU_SUB + 3] + col[PU_DEL];
	uint32_t alt = 0, kind = 6;
	for (uint32_t k = 0; k < 6; ++k)
	{
		if (k == ref) continue;
		const uint32_t v = k < 4 ? col[PU_SUB + k] : col[PU_DEL + (k - 4)];
		if (kind == 6 || v > alt) { alt = v; kind = k; }
	}
	if (depth < T.min_depth || alt < T.min_alt || (uint64_t)alt * 1000 < (uint64_t)T.min_permille * depth) return false;
	const uint32_t s = pile_seq_of(G.seq_base, G.n_seqs, x);
	o.seq = s; o.pos = (uint32_t)(x - G.seq_base[s]); o.ref = ref; o.kind = kind; o.match = col[PU_MATCH];
	o.sub[0] = col[PU_SUB]; o.sub[1] = col[PU_SUB + 1]; o.sub[2] = col[PU_SUB + 2]; o.sub[3] = col[PU_SUB + 3];
	o.del = col[PU_DEL]; o.ins = col[PU_INS]; o.depth = depth > OV_POS_MAX ? (uint32_t)OV_POS_MAX : (uint32_t)depth;
	return true;
}

// ---- the host twin --------------------------------------------------------------------------------------------------------------------
struct PileHost {
	std::vector<uint32_t> piece_first, origin; std::vector<uint64_t> seq_base;
	PileGeom G{};
	std::vector<uint32_t> cols, diff;                                          // n_pos * PU_COLS; n_pos + 1
	cl_pileup_sums sums{};
	cl_status init(const uint64_t* seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap)
	{
		const cl_status s = pile_geometry(seq_len, n_seqs, read_len, overlap, piece_first, seq_base, origin);
		if (s != CL_OK) return s;
		G = PileGeom{ seq_base.data(), piece_first.data(), origin.data(), seq_base[n_seqs], n_seqs, piece_first[n_seqs], read_len, read_len - overlap };
		cols.assign((size_t)G.n_pos * PU_COLS, 0); diff.assign((size_t)G.n_pos + 1, 0);
		return CL_OK;
	}
};
// The visitor of es_walk_host: the cursor, the reference and W.last for the run rule are the walk's, and so is every check.
struct PileHostVisitor {
	PileHost& H;
	bool touched = false;
	void plain(uint32_t, uint64_t) {}
	void begin(const EsHostWalk&) { touched = false; }
	void tuple(const EsHostWalk& W, uint32_t t, uint32_t v, uint32_t val, uint32_t rb)
	{
		if (t > T_SKIP || W.cur.id >= H.G.n_pseudo) return;
		touched = true;
		const uint64_t o = H.origin[W.cur.id]; const uint32_t len = (uint32_t)W.cur.len; const bool rev = W.cur.rev;
		uint64_t p = 0;
		switch (t)
		{
		case T_INS:
			if (W.last == T_INS) break;                                        // the run is booked where it opened
			if (pile_ins_left(o, len, rev, W.cursor, p)) H.cols[p * PU_COLS + PU_INS] += 1; else H.sums.ins_unplaced += 1;
			break;
		case T_DEL: H.cols[pile_at(o, len, rev, W.cursor) * PU_COLS + PU_DEL] += 1; break;
		case T_MATCH: H.cols[pile_at(o, len, rev, W.cursor) * PU_COLS + PU_MATCH] += 1; break;
		case T_SUBST: H.cols[pile_at(o, len, rev, W.cursor) * PU_COLS + PU_SUB + pile_sub_base(rb, v, rev)] += 1; break;
		case T_ANCHOR:
			if (val) { p = pile_anchor_start(o, len, rev, W.cursor, val); H.diff[p] += 1; H.diff[p + val] -= 1; }
		}
	}
	uint32_t end(const EsHostWalk&, uint64_t) { if (touched) H.sums.reads += 1; return EDE_NONE; }
};
// the streams of a batch added.  false: a malformed stream — *bad_read / *bad_code name the first — and the table is spoiled
inline bool pile_add_host(PileHost& H, const uint8_t* ref_codes, const uint64_t* ref_off, uint32_t n_refs, const uint8_t* es, const uint64_t* es_off, uint64_t n_reads,
                          uint64_t* bad_read, uint32_t* bad_code)
{
	PileHostVisitor vis{ H };
	return es_walk_host(ref_codes, ref_off, n_refs, n_refs, es, es_off, n_reads, true, vis, bad_read, bad_code);
}
// the fold: the running sum of diff into `match`, `ref` from the pieces, the totals
inline void pile_fold_host(PileHost& H, const uint8_t* ref_codes, const uint64_t* ref_off)
{
	uint32_t run = 0;
	for (uint64_t x = 0; x < H.G.n_pos; ++x)
	{
		uint32_t* col = &H.cols[x * PU_COLS];
		run += H.diff[x];
		col[PU_MATCH] += run;
		uint32_t id, off; pile_ref_place(H.G, x, id, off);
		col[PU_REF] = ref_codes[ref_off[id] + off] & 3u;
		const uint64_t sub = (uint64_t)col[PU_SUB] + col[PU_SUB + 1] + col[PU_SUB + 2] + col[PU_SUB + 3];
		if (col[PU_MATCH] || sub || col[PU_DEL]) H.sums.covered += 1;
		H.sums.match += col[PU_MATCH]; H.sums.sub += sub; H.sums.del += col[PU_DEL]; H.sums.ins += col[PU_INS];
	}
}
inline void pile_sites_host(const PileHost& H, const PileThresholds& T, std::vector<cl_pileup_site>& out)
{
	cl_pileup_site o;
	for (uint64_t x = 0; x < H.G.n_pos; ++x) if (pile_site(H.G, x, &H.cols[x * PU_COLS], T, o)) out.push_back(o);
}
