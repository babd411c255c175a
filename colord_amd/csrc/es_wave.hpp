// es_wave.hpp — the tuple stream of one read walked by one wave: what k_es_expand (expand.hip), k_edit_profile (edits.hip),
// k_overlap_walk (overlaps.hip), k_pileup_walk (pileup.hip) and k_cigar_walk (cigars.hip) share.  The format, the codes and the order of the checks are es_codes.hpp's, as the host walk has them.
//
// The wave takes the stream 64 bytes at a time, one byte per lane.  Per window (es_window):
//   1. tuple starts: a tuple is 1, 4 or 5 bytes long by its type nibble, and payload bytes look like anything, so the starts are a chain
//      — walked as a UNIFORM loop over three 64-bit ballots (one-byte types, four-byte, five-byte): a run of one-byte tuples is one step
//      (count-trailing-zeros), a multi-byte tuple one step: at most 2 x 16 steps per window, none per lane.  A multi-byte tuple that
//      crosses the window's end starts the next window.
//   2. every start lane has its tuple's payload by four lane shifts, and from it what the tuple advances the reference cursor and the read
//      position by (es_ref_adv, es_read_adv).
// Alt-id / main-ref tuples cut the window into stretches that share a reference (rare: a uniform loop over their ballot, es_stretch /
// es_behind); within a stretch the kernels place every tuple by wave prefix sums of the advances.  What a kernel does per window and per
// stretch stays in its own file.  EsRefs is the reference state: the cursors on the main and the current reference and the table
// "alternative id -> orientation of its first appearance" (at most 64 entries) in one VGPR pair: lane i holds entry i.
//
// Bounds by construction: a window never holds a byte at or past the stream's end and a tuple that would cross it is an error; every
// reference id is checked against the arena's read count before its length is loaded; every reference base comes through ref_base(),
// which answers 255 outside the read (an error, never an access); a 65th alternative is an error.
#pragma once
#include "common.hpp"
#include "es_codes.hpp"

// the reference reads (lens, n) and, for the kernels that load bases, their packed words; inv: the N masks of an arena of input reads
struct Arena { const uint64_t* packed; const uint32_t* inv; const uint64_t* word_off; const uint32_t* lens; uint32_t n; };
struct RefCursor { uint32_t id = 0, len = 0; uint64_t wo = 0; bool rev = false; };
// GetRefRead(id, rev)[pos] with the guard 255 (reference_reads.h:142-207); `c` was made from an id below the arena's read count
__device__ __forceinline__ uint32_t ref_base(const Arena& R, const RefCursor& c, uint64_t pos)
{
	if (pos >= c.len) return 255;
	const uint32_t p = c.rev ? c.len - 1 - (uint32_t)pos : (uint32_t)pos;
	const uint32_t b = (uint32_t)(R.packed[c.wo + (p >> 5)] >> (62 - 2 * (p & 31))) & 3u;
	return c.rev ? 3u - b : b;
}

// the lowest lane's code among the lanes that have one (uniform), or EDE_NONE
__device__ __forceinline__ uint32_t es_lane_err(uint32_t lane_err)
{
	const uint64_t le = __ballot(lane_err != EDE_NONE);
	return le ? __builtin_amdgcn_readfirstlane(__shfl(lane_err, (uint32_t)__builtin_ctzll(le), 64)) : (uint32_t)EDE_NONE;
}

// The start tuple of the n > 0 stream bytes at s (uniform): five lanes load it.  err: plain kinds have none; else START, then n < 5 ->
// TRUNC, then the id against the n_refs reference reads -> REF_ID.
struct EsStart { uint32_t t0, main_id, err; bool plain, rev; };
__device__ __forceinline__ EsStart es_start(const uint8_t* __restrict__ s, uint64_t n, uint32_t lane, uint32_t n_refs)
{
	const uint32_t hb = lane < 5 && lane < n ? (uint32_t)s[lane] : 0u;
	const uint32_t b0 = __builtin_amdgcn_readfirstlane(hb);
	EsStart st;
	st.t0 = b0 >> 4; st.rev = (b0 & 0xf) != 0; st.plain = st.t0 == T_START_PLAIN || st.t0 == T_START_PLAIN_N;
	st.main_id = __builtin_amdgcn_readfirstlane((__shfl(hb, 1, 64) << 24) | (__shfl(hb, 2, 64) << 16) | (__shfl(hb, 3, 64) << 8) | __shfl(hb, 4, 64));
	st.err = st.plain ? EDE_NONE : st.t0 != T_START_ES ? EDE_START : n < 5 ? EDE_TRUNC : st.main_id >= n_refs ? EDE_REF_ID : EDE_NONE;
	return st;
}

// a byte behind a plain start tuple: what is wrong with it
__device__ __forceinline__ uint32_t es_plain_err(uint32_t b) { return (b >> 4) != T_PLAIN ? EDE_TYPE : (b & 0xf) > 4 ? EDE_VALUE : EDE_NONE; }
// the rest of a plain stream checked, a lane per base: my lane's code
__device__ __forceinline__ uint32_t es_plain_check(const uint8_t* __restrict__ s, uint64_t n, uint32_t lane)
{
	uint32_t lane_err = EDE_NONE;
	for (uint64_t i = 1 + lane; i < n; i += 64) { const uint32_t e = es_plain_err(s[i]); if (e) lane_err = e; }
	return lane_err;
}

// One window: the wn = min(64, n - pos) bytes at s + pos.  b / t: my byte (0xff past wn) and its type; m5: the lanes with an alt-id type;
// starts: the lanes where a tuple starts, p: the bytes that whole tuples take (the next window begins behind them); for a start lane
// v28 / id32: its 28-bit value / 32-bit id (a start's payload is inside the window).  err: TYPE, or TRUNC when no whole tuple fits
// (a window of 64 bytes holds any tuple: this one ends past the stream).
struct EsWindow { uint32_t wn, b, t, p, v28, id32, err; uint64_t m5, starts; bool is_start; };
__device__ __forceinline__ EsWindow es_window(const uint8_t* __restrict__ s, uint64_t pos, uint64_t n, uint32_t lane)
{
	EsWindow W;
	// never a byte at or past the stream's end.  pos and n are the wave's, uniform, and the compiler is told so here: with that the loop
	// over the ballots below, p, starts and what the kernels derive from them (the stretch loop) are scalar code
	W.wn = __builtin_amdgcn_readfirstlane(n - pos < 64 ? (uint32_t)(n - pos) : 64u);
	W.b = lane < W.wn ? (uint32_t)s[pos + lane] : 0xffu;
	W.t = W.b >> 4;
	const uint32_t wn = W.wn, t = W.t;
	const uint64_t m1 = __ballot(lane < wn && (t <= T_SUBST || t == T_MAIN_REF));
	const uint64_t m4 = __ballot(lane < wn && (t == T_ANCHOR || t == T_SKIP));
	W.m5 = __ballot(lane < wn && t == T_ALT_ID);
	uint64_t starts = 0; uint32_t p = 0, err = EDE_NONE;
	while (p < wn)
	{
		const uint64_t bit = 1ull << p;
		if (m1 & bit)
		{	// the run of one-byte tuples from here
			const uint64_t z = ~(m1 >> p);
			const uint32_t k = z ? (uint32_t)__builtin_ctzll(z) : 64u;
			starts |= (k >= 64 ? ~0ull : (1ull << k) - 1) << p; p += k;
		}
		else if (m4 & bit) { if (p + 4 > wn) break; starts |= bit; p += 4; }
		else if (W.m5 & bit) { if (p + 5 > wn) break; starts |= bit; p += 5; }
		else { err = EDE_TYPE; break; }
	}
	if (!err && p == 0) err = EDE_TRUNC;
	W.starts = starts; W.p = p; W.err = err;
	W.is_start = (starts >> lane) & 1;
	const uint32_t b1 = __shfl_down(W.b, 1, 64), b2 = __shfl_down(W.b, 2, 64), b3 = __shfl_down(W.b, 3, 64), b4 = __shfl_down(W.b, 4, 64);
	W.v28 = ((W.b & 0xf) << 24) | (b1 << 16) | (b2 << 8) | b3;
	W.id32 = (b1 << 24) | (b2 << 16) | (b3 << 8) | b4;
	return W;
}
// what my tuple advances the reference cursor / the read position (the bases it gives) by; 0 where no tuple starts
__device__ __forceinline__ uint32_t es_ref_adv(const EsWindow& W)
{
	return !W.is_start ? 0u : (W.t == T_DEL || W.t == T_MATCH || W.t == T_SUBST) ? 1u : (W.t == T_ANCHOR || W.t == T_SKIP) ? W.v28 : 0u;
}
__device__ __forceinline__ uint32_t es_read_adv(const EsWindow& W)
{
	return !W.is_start ? 0u : (W.t == T_INS || W.t == T_MATCH || W.t == T_SUBST) ? 1u : W.t == T_ANCHOR ? W.v28 : 0u;
}

// The stretch step.  todo: the tuple starts of the window not yet taken; sw: those that change the reference (alt-id, main-ref).
// seg: the tuples of the next stretch, all on the current reference; sl: the lane of the tuple that ends it, 64 when the window does.
struct EsStretch { uint32_t sl; uint64_t seg; };
__device__ __forceinline__ EsStretch es_stretch(uint64_t todo, uint64_t sw)
{
	const uint64_t swm = todo & sw;
	EsStretch x;
	x.sl = swm ? (uint32_t)__builtin_ctzll(swm) : 64u;
	x.seg = x.sl >= 64 ? todo : todo & ((1ull << x.sl) - 1);
	return x;
}
// todo behind the tuple at sl < 64
__device__ __forceinline__ uint64_t es_behind(uint64_t todo, uint32_t sl) { return todo & ~(((1ull << sl) << 1) - 1); }

// The reference state of a read (uniform, but the table).  BASES: the kernel loads reference bases, so a cursor carries its word offset.
template<bool BASES> struct EsRefs {
	RefCursor mainc, cur;
	uint64_t cursor = 0, main_cursor = 0; bool is_main = true;
	uint32_t n_alt = 0, my_alt_id = 0, my_alt_rev = 0;                          // lane i: alternative i of this read and the orientation it came with first
	static __device__ __forceinline__ RefCursor at(const Arena& R, uint32_t id, bool rev)
	{	// id < R.n
		RefCursor c; c.id = id; c.len = R.lens[id]; if (BASES) c.wo = R.word_off[id]; c.rev = rev;
		return c;
	}
	__device__ __forceinline__ EsRefs(const Arena& R, const EsStart& st) { mainc = cur = at(R, st.main_id, st.rev); }
	// a main-ref tuple: back to the main reference where it was left
	__device__ __forceinline__ void to_main() { if (!is_main) { cur = mainc; cursor = main_cursor; is_main = true; } }
	// an alt-id tuple with this (uniform) id and orientation nibble: the error, or EDE_NONE and the cursor at the alternative's start
	__device__ __forceinline__ uint32_t to_alt(const Arena& R, uint32_t id, uint32_t orient, uint32_t lane)
	{
		if (id >= R.n) return EDE_REF_ID;
		if (is_main) { main_cursor = cursor; is_main = false; }
		const uint64_t hit = __ballot(lane < n_alt && my_alt_id == id);
		uint32_t rev;
		if (hit) rev = __shfl(my_alt_rev, (uint32_t)__builtin_ctzll(hit), 64);      // the orientation of its first appearance holds
		else
		{
			if (n_alt >= ED_MAX_ALT) return EDE_TOO_MANY_ALT;
			if (lane == n_alt) { my_alt_id = id; my_alt_rev = orient; }
			++n_alt; rev = orient;
		}
		cur = at(R, id, __builtin_amdgcn_readfirstlane(rev) != 0);
		cursor = 0;
		return EDE_NONE;
	}
	// the alt-id tuple at lane sl of window W
	__device__ __forceinline__ uint32_t to_alt(const Arena& R, const EsWindow& W, uint32_t sl, uint32_t lane)
	{
		return to_alt(R, __builtin_amdgcn_readfirstlane(__shfl(W.id32, sl, 64)), (__shfl(W.b, sl, 64) & 0xf) != 0 ? 1u : 0u, lane);
	}
};
