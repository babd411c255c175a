// gap_tail.hpp — the tail of a level: what the decisions, the estimator and the tuple emission need of every gap's finished script, made
// in ONE pass over the script by a group of lanes (device only).
//
// Per gap (gap_finish / gap_stats / analyze_es / gap_summary of encode_core.hpp are the sequential statement):
//   - a trivial gap gets its script (the read's bases as letters) or its d_before;
//   - ne <  min_part_alt: the PendRec the adaptive estimator decides from later (run statistics of d_before x 'D' + script, base counts);
//   - ne >= min_part_alt: the static entropy decision (EncodeWithEditScript, encoder.cpp:1315-1327) and the spawn flag;
//   - es_len > 0: the GapSum of the script for the count pass of the emission.
// A lane takes 8 script symbols (one 8-byte load).  A ballot of the lanes in which a run STARTS gives every lane, with one shuffle, the
// run that is open where its symbols begin (the nearest such lane below it, whole words of one symbol in between; before the group's
// first lane: the run carried over from the step before).  The lane then accounts every run that ENDS at one of its symbols — the first
// run of the script as the summary's first_len, the others as bytes / tuples of the middle, for a short gap the estimator's run
// statistics — and the script's last run is accounted after the loop.  Symbol counts go through 4-bit counters packed in a 64-bit word.
// W = 16: a ROW per gap, four gaps per wave (k_gap_tail; the row idiom of k_align_quad_rows: all control flow is row-uniform and every
// shuffle stays inside the row).  W = 64: a wave per gap, for the scripts beyond the row limit (k_gap_stats_long).
#pragma once
#include "emit_wave.hpp"

namespace enc {

// the RunEl of up to eight symbols held in the low bytes of w (nb = 1 .. 8; the bytes above are zero, which no symbol is).  Runs inside
// a word are shorter than any 4-byte tuple, so what closes strictly inside puts out a byte and a tuple per symbol
__device__ inline RunEl run_of_word(uint64_t w, uint32_t nb)
{
	const uint32_t f = (uint32_t)w & 0xffu, l = (uint32_t)(w >> (8 * (nb - 1))) & 0xffu;
	const uint64_t xf = w ^ (0x0101010101010101ull * f);
	uint32_t hl = xf ? (uint32_t)__builtin_ctzll(xf) >> 3 : 8u;
	if (hl >= nb) return run_single(f, nb);
	const uint64_t xl = (w << (8 * (8 - nb))) ^ (0x0101010101010101ull * l);    // the symbols in the top bytes; not one run, so xl != 0
	const uint32_t tl = (uint32_t)__builtin_clzll(xl) >> 3;
	return RunEl{ f, hl, l, tl, nb - hl - tl, nb - hl - tl, 0 };
}
template<int W> __device__ inline uint32_t group_sum(uint32_t v)
{
#pragma unroll
	for (int o = W / 2; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
	return v;
}

// a finished run of the estimator's view (analyze_es): dm = { symbols of short D runs, of short M runs, long D runs, long M runs };
// returns the (ilog2(len) + 1) + 1 term of a long run for `lens`, else 0
__device__ inline uint32_t tail_close_run(uint32_t sym, uint32_t len, uint32_t (&dm)[4])
{
	if (sym == (uint32_t)'D') { if (len >= 10) { ++dm[2]; return bitlen32(len) + 1; } dm[0] += len; }
	else if (sym == (uint32_t)'M') { if (len >= 15) { ++dm[3]; return bitlen32(len) + 1; } dm[1] += len; }
	return 0;
}

// the fields of a gap's record the tail sets (the others stay as they are in memory: the lanes need not hold them)
__device__ inline void tail_store_gap(GapRec& dst, const GapRec& g, uint32_t state, uint32_t aux)
{
	dst.d_before = g.d_before; dst.es_len = g.es_len; dst.state = state; dst.aux = aux;
}

// One gap by a group of W lanes.  g: the gap's record as the aligners left it (every lane holds it); pend_slot: its slot in L.pend when
// the estimator decides it.  SUMS: the group also writes the script's GapSum.
template<int W, bool SUMS>
__device__ inline void gap_tail_group(const LevelV& L, const ArenaV& A, const EncCfg& cfg, uint32_t gi, GapRec g, uint32_t pend_slot,
                                      GapSum* __restrict__ sums, uint32_t* __restrict__ spawn_flag)
{
	const uint32_t gl = threadIdx.x & (W - 1), group_at = (threadIdx.x & 63u) & ~(uint32_t)(W - 1);
	char* es = L.es + g.es_off;
	const uint64_t ewb = A.word_off[g.read];
	// get_edit_dist_on_seq_empty (edit_script.h:250-267): the lanes make the letters they then work on, so nothing is read back
	const bool letters = g.kind == GK_TRIVIAL && g.nr == 0;
	if (g.kind == GK_TRIVIAL) { if (g.nr == 0) g.es_len = g.ne; else g.d_before = g.nr; }
	const bool pending = g.ne < cfg.min_part_alt;
	const uint32_t k = g.es_len;
	// static decision: h = the script's symbols by class (es_class).  Pending: h = the RUNS by the class of their symbol (the estimator
	// counts a run of anything but D / M once), dm / lens = the D and M runs by their length.  Both: what the summary needs
	uint32_t h[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, hd[4] = { 0, 0, 0, 0 }, dm[4] = { 0, 0, 0, 0 };
	uint32_t first_len = 0, mid_b = 0, mid_t = 0, head_sym = 0;
	uint32_t carry_sym = 0, carry_len = 0;                                       // the run open at the end of the steps so far (group-uniform)
	uint64_t lens = 0;
	for (uint32_t x0 = 0; x0 < k; x0 += 8 * W)
	{
		const uint32_t x = x0 + gl * 8;
		uint64_t w = 0; uint32_t nb = 0;
		if (x < k)
		{
			nb = k - x < 8 ? k - x : 8;
			if (letters)
			{
				for (uint32_t y = 0; y < nb; ++y) w |= (uint64_t)(uint8_t)base_letter(arena_base_at(A, ewb, g.enc_start + x + y)) << (8 * y);
				if (nb == 8) __builtin_memcpy(es + x, &w, 8);
				else for (uint32_t y = 0; y < nb; ++y) es[x + y] = (char)((w >> (8 * y)) & 0xffu);
			}
			else if (nb == 8) __builtin_memcpy(&w, es + x, 8);
			else for (uint32_t y = 0; y < nb; ++y) w |= (uint64_t)(uint8_t)es[x + y] << (8 * y);
		}
		const RunEl e = nb ? run_of_word(w, nb) : run_empty();
		if (x0 == 0) head_sym = (uint32_t)__shfl((int)e.hs, 0, W);
		// the run open where the lane's symbols start: symbol = the last one of the lane below; a run STARTS in a lane unless the lane is
		// one run that continues that symbol; below the lane, above the nearest lane with a start, every lane is eight symbols of it
		uint32_t osym = (uint32_t)__shfl_up((int)e.ts, 1, W);
		if (gl == 0) osym = carry_sym;
		const bool starts = nb && !(e.single && e.hs == osym);
		const uint64_t below = ((__ballot(starts) >> group_at) & (W == 64 ? ~0ull : (1ull << (W & 63)) - 1)) & ((1ull << gl) - 1);
		const uint32_t at = below ? 63u - (uint32_t)__builtin_clzll(below) : 0u;
		const uint32_t tl_at = (uint32_t)__shfl((int)e.tl, (int)at, W);
		uint32_t olen = below ? tl_at + 8 * (gl - 1 - at) : carry_len + 8 * gl, long_term = 0;
		if (pending && x == 0 && g.d_before && e.hs != (uint32_t)'D') long_term = tail_close_run((uint32_t)'D', g.d_before, dm);   // d_before x 'D' is a run of its own
		const uint64_t code4 = ((w ^ (w >> 4)) & 0x0f0f0f0f0f0f0f0full) << 2;       // per byte 4 x a code that tells the nine symbols apart
		uint64_t cnt = 0;                                                         // sixteen 4-bit counters: at most 8 per step
#pragma unroll
		for (int j = 0; j < 8; ++j)
		{
			if (j >= (int)nb) break;
			const uint32_t c = (uint32_t)(w >> (8 * j)) & 0xffu;
			const bool nw = c != osym;
			if (nw)
			{
				if (olen)
				{	// the run (osym, olen) ends here; it started at script position x + j - olen
					const bool first = x + j == olen;
					if (first) first_len = olen; else { mid_b += run_bytes((char)osym, olen); mid_t += run_tuples((char)osym, olen); }
					if (pending)
					{	// (at most one long run ends in a lane's eight symbols: the one it inherited)
						const uint32_t t = tail_close_run(osym, olen + (first && osym == (uint32_t)'D' ? g.d_before : 0u), dm);
						if (t) long_term = t;
					}
				}
				osym = c; olen = 0;
			}
			++olen;
			if (!pending || nw) cnt += 1ull << ((uint32_t)(code4 >> (8 * j)) & 63u);
		}
		// code = (c ^ c >> 4) & 15: A 5, C 7, D 0, G 3, M 9, T 1, X 13, Y 12, Z 15
		h[0] += (uint32_t)(cnt >> 20) & 15u; h[1] += (uint32_t)(cnt >> 28) & 15u; h[2] += (uint32_t)cnt & 15u; h[3] += (uint32_t)(cnt >> 12) & 15u;
		h[4] += (uint32_t)(cnt >> 36) & 15u; h[5] += (uint32_t)(cnt >> 4) & 15u; h[6] += (uint32_t)(cnt >> 52) & 15u; h[7] += (uint32_t)(cnt >> 48) & 15u;
		h[8] += (uint32_t)(cnt >> 60) & 15u;
		const uint32_t last_lane = (k - x0 - 1) >> 3 < (uint32_t)(W - 1) ? (k - x0 - 1) >> 3 : (uint32_t)(W - 1);
		carry_sym = (uint32_t)__shfl((int)osym, (int)last_lane, W); carry_len = (uint32_t)__shfl((int)olen, (int)last_lane, W);
		if (pending)
		{	// lens_push depends on the order: the lanes' long runs in lane order, by every lane of the group alike (they are rare)
			uint64_t m = (__ballot(long_term != 0) >> group_at) & (W == 64 ? ~0ull : (1ull << (W & 63)) - 1);
			while (m) { lens_push(lens, (uint32_t)__shfl((int)long_term, (int)__builtin_ctzll(m), W)); m &= m - 1; }
		}
	}
	if (g.ne)
	{	// the read's bases a packed word (32 bases) per lane and load, counted by popcounts
		const uint32_t s = g.enc_start, last = g.enc_start + g.ne - 1, w0 = s >> 5, w1 = last >> 5;
		for (uint32_t wi = w0 + gl; wi <= w1; wi += W)
		{
			const uint64_t w = A.packed[ewb + wi];
			const uint32_t ja = wi == w0 ? (s & 31) : 0u, jb = wi == w1 ? (last & 31) : 31u;    // fields (bases) ja .. jb of the word count; base j sits at bits 63 - 2 j, 62 - 2 j
			const uint64_t from = ja == 0 ? ~0ull : ((1ull << (64 - 2 * ja)) - 1), upto = ~((1ull << (62 - 2 * jb)) - 1);
			const uint64_t v = from & upto & 0x5555555555555555ull, lo = w & 0x5555555555555555ull, hi = (w >> 1) & 0x5555555555555555ull;
			const uint32_t c3 = (uint32_t)__popcll(lo & hi & v), c2 = (uint32_t)__popcll(hi & ~lo & v), c1 = (uint32_t)__popcll(lo & ~hi & v);
			hd[3] += c3; hd[2] += c2; hd[1] += c1; hd[0] += (uint32_t)__popcll(v) - c1 - c2 - c3;
		}
	}
#pragma unroll
	for (int q = 0; q < 9; ++q) h[q] = group_sum<W>(h[q]);
#pragma unroll
	for (int q = 0; q < 4; ++q) hd[q] = group_sum<W>(hd[q]);
	const bool one_run = k && carry_len == k;                                    // the script's last run is its first
	if (!one_run) { first_len = group_sum<W>(first_len); mid_b = group_sum<W>(mid_b); mid_t = group_sum<W>(mid_t); }
	else { first_len = k; mid_b = mid_t = 0; }
	if (SUMS && k && gl == 0) sums[gi] = GapSum{ first_len, carry_len, mid_b, mid_t, head_sym | (carry_sym << 8) | (one_run ? 1u << 16 : 0u) };
	if (pending)
	{
#pragma unroll
		for (int q = 0; q < 4; ++q) dm[q] = group_sum<W>(dm[q]);
		// the script's last run ends here (with the d_before deletions when it is the first one too; they alone when there is no script)
		uint32_t t = 0;
		if (k) t = tail_close_run(carry_sym, carry_len + (one_run && carry_sym == (uint32_t)'D' ? g.d_before : 0u), dm);
		else if (g.d_before) t = tail_close_run((uint32_t)'D', g.d_before, dm);
		if (t) lens_push(lens, t);
		if (gl == 0)
		{	// est_code order A C G T D M X Y Z . . from es_class order A C D G M T X Y Z
			PendRec p;
			p.rd[0] = h[0]; p.rd[1] = h[1]; p.rd[2] = h[3]; p.rd[3] = h[5]; p.rd[4] = dm[0]; p.rd[5] = dm[1];
			p.rd[6] = h[6]; p.rd[7] = h[7]; p.rd[8] = h[8]; p.rd[9] = dm[2]; p.rd[10] = dm[3]; p.rd[11] = 0;
			p.pl[0] = hd[0]; p.pl[1] = hd[1]; p.pl[2] = hd[2]; p.pl[3] = hd[3];
			p.ref_len = g.nr; p.pad = 0; p.lens = lens;
			L.pend[pend_slot] = p;
			tail_store_gap(L.gaps[gi], g, GS_PENDING, pend_slot); spawn_flag[gi] = 0u;
		}
		return;
	}
	// EncodeWithEditScript (encoder.cpp:1315-1327) with GetEditScriptEntropyInput (:1299-1311): the script is scored without its leading deletions
	const uint32_t nd = k && head_sym == (uint32_t)'D' ? first_len : 0u;
	uint32_t n = g.es_len, extra = g.d_before;
	if (nd + g.d_before >= 10) { h[2] -= nd; n -= nd; extra = 0; }
	h[2] += extra;
	// the two entropies (entropy_hist, encode_core.hpp): their thirteen p log2 p terms one per lane in ONE evaluation of the logarithm (lanes
	// 0 .. 8 the script's classes, 9 .. 12 the bases); the sums run over the terms in the sequential order, so the doubles are the sequential ones
	double sum_h = 0, sum_d = 0;
#pragma unroll
	for (int i = 0; i < 9; ++i) sum_h += h[i];
#pragma unroll
	for (int i = 0; i < 4; ++i) sum_d += hd[i];
	const double rec_h = 1.0 / sum_h, rec_d = 1.0 / sum_d;
	constexpr int ROUNDS = (13 + W - 1) / W;                                     // (a group of 8 lanes takes two terms a lane)
	double term[ROUNDS];
#pragma unroll
	for (int r = 0; r < ROUNDS; ++r)
	{
		const uint32_t idx = gl + (uint32_t)(r * W);
		uint32_t mine = 0;
#pragma unroll
		for (int i = 0; i < 9; ++i) if (idx == (uint32_t)i) mine = h[i];
#pragma unroll
		for (int i = 0; i < 4; ++i) if (idx == 9u + (uint32_t)i) mine = hd[i];
		term[r] = 0;
		if (mine) { const double p = (double)mine * (idx < 9 ? rec_h : rec_d); term[r] = glibc_log2::log2(p) * p; }
	}
	double e_h = 0, e_d = 0;
#pragma unroll
	for (int i = 0; i < 9; ++i) { const double t = __shfl(term[i / W], i % W, W); if (h[i]) e_h += t; }
#pragma unroll
	for (int i = 0; i < 4; ++i) { const double t = __shfl(term[(9 + i) / W], (9 + i) % W, W); if (hd[i]) e_d += t; }
	const bool accept = -e_h * (double)(n + extra) * cfg.cost_mult < -e_d * (double)g.ne;
	if (gl == 0) { tail_store_gap(L.gaps[gi], g, accept ? GS_ES : GS_REJECTED, g.aux); spawn_flag[gi] = accept ? 0u : 1u; }
}

} // namespace enc
