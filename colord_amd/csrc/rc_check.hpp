// rc_check.hpp — the DECODER's interval arithmetic (sub_rc.h:216-392) against known triples: does a coded part decode to the
// intervals the models gave its symbols, and does it end at its size?  The opt-in check behind cl_ctx_set_verify_streams.
//
// A part is checked by ONE lane, as k_range_code (rc_dev.hpp) codes it: the decoder's (low, range) follow the triples alone — they are
// the coder's own — and only `buffer` follows the bytes, so the chain per symbol is the coder's with a comparison in place of the byte
// ring.  What is NOT replayed: the models.  The triples are taken as the models made them; a decoder that evolves its own models from
// the decoded symbols stays on the host (decode.hip).
//
// The step of one symbol (check, update, renormalise against a byte source) is written once, rc_check_step, for the kernel and for
// host loops: with RC_CHECK_HOST_ONLY defined this header needs no HIP at all (tests/tools/rc_check_host_test.cpp).
#pragma once
#include <stdint.h>
#ifdef RC_CHECK_HOST_ONLY
#define RC_HD
#else
#include "rc_dev.hpp"
#define RC_HD __host__ __device__
#endif

constexpr uint64_t RC_TOP = 0x00ffffffffffffULL, RC_MASK = 0xff00000000000000ULL;
constexpr uint32_t RC_DECODES = 0xffffffffu;                                // first_bad of a part that decodes

RC_HD inline uint64_t rc_mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __umul64hi(a, b);
#else
	return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// range / tot as in k_range_code, inv = floor((2^64-1) / tot): the high product is the quotient or one below it, the remainder it
// leaves is below 2 tot < 2^22.  (The decoder's `range /= tot` of GetCumulativeFreq, sub_rc.h:264-268; a decoder that has to FIND its
// symbol — k_qual_decode — compares q t <= buffer for the cumulative counts t before it takes the step below.)
RC_HD inline uint64_t rc_quotient(uint64_t range, uint32_t tot, uint64_t inv)
{
	uint64_t q = rc_mulhi64(range, inv);
	const uint32_t rem = (uint32_t)range - (uint32_t)q * tot;
	return q + (uint32_t)(rem >= tot);
}

// One symbol of the decoder (sub_rc.h:264-286) whose interval is known: t = cum << 42 | freq << 21 | tot, inv = floor((2^64-1) / tot).
// false: the symbol does not decode — a triple that is no interval (tot == 0, freq == 0, cum + freq > tot; nothing is computed from it),
// or a buffer outside the symbol's interval: with q = range / tot, cum <= buffer / q < cum + freq  <=>  q cum <= buffer < q (cum + freq)
// (q freq <= range: no overflow), GetCumulativeFreq's value inside [cum, cum + freq) without the second division.  Nothing is changed then.
// Src: peek8() = the next 8 bytes of the part, big-endian, zeros where the part has none; advance(n), n <= 8.  The renormalisation
// does not depend on the bytes, so its steps are counted first and the bytes taken in one piece.  Like the coder's it stops after 8
// steps: nothing of low is left then, and a range that is still not above TOP (it is 0: corrupt triples, k_range_code reports such a
// part as overflowing) fails the symbol.
template<class Src>
RC_HD inline bool rc_check_step(uint64_t& low, uint64_t& range, uint64_t& buffer, uint64_t t, uint64_t inv, Src& src)
{
	const uint32_t tot = (uint32_t)(t & 0x1fffff), freq = (uint32_t)((t >> 21) & 0x1fffff), cum = (uint32_t)(t >> 42);
	if (tot == 0 || freq == 0 || cum + freq > tot) return false;
	const uint64_t q = rc_quotient(range, tot, inv);
	const uint64_t r = q * cum;
	if (buffer < r || buffer - r >= q * freq) return false;
	buffer -= r; low += r; range = q * freq;
	uint32_t nb = 0;
	while (range <= RC_TOP && nb < 8)
	{
		if ((low ^ (low + range)) & RC_MASK) range = (low | RC_TOP) - low;      // cut at a straddled top-byte boundary
		low <<= 8; range <<= 8; ++nb;
	}
	if (nb)
	{
		const uint64_t w = src.peek8();
		buffer = nb == 8 ? w : (buffer << (8 * nb)) | (w >> (64 - 8 * nb));
		src.advance(nb);
	}
	return range > RC_TOP;
}

// The bytes of a part in host memory: bytes at or past `size` read as 0.  pos counts the bytes REQUESTED, whether or not they exist.
struct RcHostBytes {
	const uint8_t* p; uint64_t size, pos;
	RC_HD void start(const uint8_t* part, uint64_t size_) { p = part; size = size_; pos = 0; }
	RC_HD uint64_t peek8() const { uint64_t w = 0; for (uint32_t i = 0; i < 8; ++i) w = (w << 8) | (pos + i < size ? p[pos + i] : 0); return w; }
	RC_HD void advance(uint32_t n) { pos += n; }
};
// The bytes of a part on the device: a lane-private window of 16 bytes (w0, w1) from index `base` of the part and the 8 bytes behind
// them on their way (nxt: loaded a refill before they are needed — the coded bytes are about 3 % of the triple traffic, so a refill
// comes every thirty symbols or so).  Every load is one unaligned 8-byte word that lies inside [0, lim): lim = the part's size once
// it was found to lie inside the buffer, else 0 — then nothing is ever loaded.  Where fewer than 8 bytes are left the word that
// ENDS at lim is loaded and shifted (lim >= 8).
// (RC_HD: the host test walks the same window over blocks of exactly a part's size.)
RC_HD inline uint64_t rc_load_be64(const uint8_t* q) { uint64_t v; __builtin_memcpy(&v, q, 8); return __builtin_bswap64(v); }   // one unaligned 8-byte load
struct RcDevBytes {
	const uint8_t* p; uint64_t lim, pos, base, w0, w1, nxt;
	RC_HD uint64_t load8(uint64_t i) const
	{
		if (i + 8 <= lim) return rc_load_be64(p + i);
		if (i >= lim) return 0;
		return rc_load_be64(p + (lim - 8)) << (8 * (uint32_t)(i + 8 - lim));
	}
	RC_HD void start(const uint8_t* part, uint64_t lim_) { p = part; lim = lim_; pos = 0; base = 0; w0 = load8(0); w1 = load8(8); nxt = load8(16); }
	RC_HD uint64_t peek8() const { const uint32_t o = (uint32_t)(pos - base); return o ? (w0 << (8 * o)) | (w1 >> (64 - 8 * o)) : w0; }
	RC_HD void advance(uint32_t n)
	{
		pos += n;
		if (pos - base >= 8) { w0 = w1; w1 = nxt; base += 8; nxt = load8(base + 16); }
	}
};

// A whole part on the host, with the result the kernel gives (used by the tests — Src = RcDevBytes walks the kernel's window — and for the message of a part that ends elsewhere).  avail: the
// bytes that exist at p (the kernel's n_bytes - part_off); *consumed (optional): the bytes the decoder asked for.
template<class Src = RcHostBytes>
inline uint32_t rc_check_part_host(const uint64_t* trip, uint32_t len, const uint8_t* p, uint64_t part_size, uint64_t avail, uint64_t* consumed = nullptr)
{
	if (consumed) *consumed = 0;
	if (part_size == ~0ULL || part_size < 8 || part_size > avail) return 0;
	Src src; src.start(p, part_size);
	uint64_t low = 0, range = RC_MASK, buffer = src.peek8();
	src.advance(8);
	for (uint32_t i = 0; i < len; ++i)
	{
		const uint32_t tot = (uint32_t)(trip[i] & 0x1fffff);
		if (!rc_check_step(low, range, buffer, trip[i], tot ? ~0ULL / tot : ~0ULL, src)) return i;
	}
	if (consumed) *consumed = src.pos;
	return src.pos == part_size ? RC_DECODES : len;
}

#ifndef RC_CHECK_HOST_ONLY
// One lane per part (by place), one wave per group of 64 parts — k_range_code's shape, triples through the same three stages
// (symbols two rounds ahead, reciprocals one round ahead, 8 symbols a round).  bytes / n_bytes: the buffer the parts lie in, part p at
// part_off[p] (any alignment, beyond 2^32) with part_size[p] bytes.  first_bad[p]: RC_DECODES, or the first symbol that does not decode,
// or part_len[p] where every symbol decodes but 8 + the renormalisation steps (the bytes a decoder asks for) differ from the size.
// A size of ~0, below 8 or reaching past n_bytes: 0.  A mismatch is an expected input: a lane that has failed goes on with the
// neutral triple and a reset state (never a renormalisation, never a load) until the wave's longest part ends.
static __global__ __launch_bounds__(64) void k_range_check(const triple_t* __restrict__ trip, const uint64_t* __restrict__ group_base,
                                                          const uint32_t* __restrict__ part_len, uint32_t n_parts,
                                                          const uint8_t* __restrict__ bytes, uint64_t n_bytes, const uint64_t* __restrict__ part_off,
                                                          const uint64_t* __restrict__ part_size, const uint64_t* __restrict__ inv_tab,
                                                          uint32_t* __restrict__ first_bad)
{
	__builtin_amdgcn_s_setprio(3);                                          // as the coder: the launch lasts as long as its slowest chain
	const uint32_t p = blockIdx.x * 64 + threadIdx.x;
	const bool live = p < n_parts;
	const uint32_t len = live ? part_len[p] : 0;
	const uint64_t off = live ? part_off[p] : 0, size = live ? part_size[p] : 0;
	const bool placed = live && size != ~0ULL && size >= 8 && off <= n_bytes && size <= n_bytes - off;
	bool ok = placed; uint32_t bad_at = 0;
	RcDevBytes src; src.start(bytes + (placed ? off : 0), placed ? size : 0);
	uint64_t low = 0, range = RC_MASK, buffer = src.peek8();
	src.advance(8);
	uint32_t lmax = len;
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) { uint32_t t = __shfl_xor(lmax, d, 64); lmax = t > lmax ? t : lmax; }
	if (lmax != 0)
	{
		const triple_t* tsrc = trip + group_base[blockIdx.x] + threadIdx.x * TRIP_RUN;   // this lane's runs: symbol q at tsrc[at(q)]
		auto at = [](uint32_t q) -> uint64_t { return (uint64_t)(q / TRIP_RUN) * (64 * TRIP_RUN) + q % TRIP_RUN; };
		constexpr uint32_t U = 8;
		static_assert(U % TRIP_RUN == 0, "a round takes whole runs of a lane's triples");
		triple_t A[U], B[U], C[U]; uint64_t iA[U], iB[U], iC[U];
		const uint64_t NEUTRAL_X = (1ULL << 21) | 1ULL, NEUTRAL_Y = ~0ULL;       // (cum 0, freq 1, total 1): range / 1 * 1, low + 0, no byte
		const uint32_t last = lmax - 1;
#pragma unroll
		for (uint32_t u = 0; u < U; ++u) { A[u] = tsrc[at(u < last ? u : last)]; B[u] = tsrc[at(U + u < last ? U + u : last)]; }
#pragma unroll
		for (uint32_t u = 0; u < U; ++u) iA[u] = inv_tab[A[u] & 0x1fffff];
		// one round: fetch `far` (two rounds ahead, index clamped to the group's longest part), look up the reciprocals of `nxt`, check `cur`
		auto round = [&](auto all_active, uint32_t pos, const triple_t (&cur)[U], const uint64_t (&icur)[U], const triple_t (&nxt)[U], uint64_t (&inxt)[U], triple_t (&far)[U])
		{
#pragma unroll
			for (uint32_t u = 0; u < U; ++u) { const uint32_t q = pos + 2 * U + u; far[u] = tsrc[at(q < last ? q : last)]; }
#pragma unroll
			for (uint32_t u = 0; u < U; ++u) inxt[u] = inv_tab[nxt[u] & 0x1fffff];
#pragma unroll
			for (uint32_t u = 0; u < U; ++u)
			{
				const bool act = ok && (decltype(all_active)::value || pos + u < len);
				const bool good = rc_check_step(low, range, buffer, act ? cur[u] : NEUTRAL_X, act ? icur[u] : NEUTRAL_Y, src);
				if (act && !good) { ok = false; bad_at = pos + u; low = 0; range = RC_MASK; buffer = 0; }   // (an idle lane's neutral step changes nothing, whatever it answers)
			}
		};
		uint32_t lmin = live ? len : 0u;
#pragma unroll
		for (int d = 32; d > 0; d >>= 1) { uint32_t t = __shfl_xor(lmin, d, 64); lmin = t < lmin ? t : lmin; }
		const std::true_type ALL{}; const std::false_type SOME{};
		uint32_t pos = 0;
		for (; pos + 3 * U <= lmin; pos += 3 * U)                                // every lane has symbols for three whole rounds
		{
			round(ALL, pos, A, iA, B, iB, C);
			round(ALL, pos + U, B, iB, C, iC, A);
			round(ALL, pos + 2 * U, C, iC, A, iA, B);
		}
		for (; pos < lmax; pos += 3 * U)
		{
			round(SOME, pos, A, iA, B, iB, C);
			if (pos + U >= lmax) break;
			round(SOME, pos + U, B, iB, C, iC, A);
			if (pos + 2 * U >= lmax) break;
			round(SOME, pos + 2 * U, C, iC, A, iA, B);
		}
	}
	if (live) first_bad[p] = !ok ? bad_at : src.pos != size ? len : RC_DECODES;
}

#define LAUNCH_RANGE_CHECK(ctx, bytes, ng, ...) LAUNCHB_NAMED(ctx, "k_range_check", bytes, k_range_check, ng, 64, __VA_ARGS__)

// ---- the check inside the coders (dna.hip, qual.hip): a group of parts right after its bytes were gathered to their final place ----
// launch: on the context's launch stream, behind the gather kernel; d_dst_off / d_size / trip / d_gbase / d_plen are the group's, by
// place; n_bytes = the extent of d_out that is written so far.  collect: after the caller's synchronisation of that stream.
struct RcCheckRun { DevBuf<uint32_t> d_first_bad; uint32_t np = 0; uint64_t n_syms = 0, part_bytes = 0; };
static inline cl_status rc_check_launch(cl_ctx* ctx, RcCheckRun& run, const triple_t* trip, const uint64_t* d_gbase, const uint32_t* d_plen, uint32_t np, uint64_t n_syms,
                                        const uint8_t* d_out, uint64_t n_bytes, uint64_t part_bytes, const uint64_t* d_dst_off, const uint64_t* d_size)
{
	const uint64_t* inv_tab = nullptr;
	CL_TRY(cl_inv_table(ctx, &inv_tab));
	run.np = np; run.n_syms = n_syms; run.part_bytes = part_bytes;
	DEV_ALLOC(ctx, run.d_first_bad, np);
	LAUNCH_RANGE_CHECK(ctx, 8.0 * n_syms + part_bytes, (np + 63) / 64, trip, d_gbase, d_plen, np, d_out, n_bytes, d_dst_off, d_size, inv_tab, run.d_first_bad.p);
	HIP_TRY(ctx, hipGetLastError());
	return CL_OK;
}
// rank: part -> place; h_part_sizes: the group's sizes in call order; p0: the group's first part in the call; dst_off: the parts'
// offsets in d_out by place.  The first bad part is the one with the smallest part index.  (A part whose symbols all decode but which
// ends elsewhere is walked once more on the host for the message's byte count: the kernel answers with one word a part.)
static inline cl_status rc_check_collect(cl_ctx* ctx, RcCheckRun& run, const char* stream_name, const triple_t* trip, const uint64_t* d_gbase, const uint32_t* d_plen,
                                         const uint8_t* d_out, const std::vector<uint64_t>& dst_off, const std::vector<uint32_t>& rank, uint32_t p0, const uint64_t* h_part_sizes)
{
	const uint32_t np = run.np;
	std::vector<uint32_t> fb(np), plen(np);                                      // by place
	HIP_TRY(ctx, hipMemcpy(fb.data(), run.d_first_bad.p, np * 4ull, hipMemcpyDeviceToHost));
	run.d_first_bad.release();
	bool bad = false;
	for (uint32_t pl = 0; pl < np; ++pl) bad |= fb[pl] != RC_DECODES;
	if (!bad)
	{
		ctx->verified_stream_parts += np; ctx->verified_stream_symbols += run.n_syms; ctx->verified_stream_bytes += run.part_bytes;
		return CL_OK;
	}
	HIP_TRY(ctx, hipMemcpy(plen.data(), d_plen, np * 4ull, hipMemcpyDeviceToHost));
	for (uint32_t p = 0; p < np; ++p)
	{
		const uint32_t pl = rank[p], at = fb[pl], n = plen[pl];
		const uint64_t size = h_part_sizes[p];
		if (at == RC_DECODES) continue;
		std::string msg = std::string("coded ") + stream_name + " stream: part " + std::to_string(p0 + p) + " (" + std::to_string(n) + " symbols, " + std::to_string(size) + " bytes) does not decode to its models' intervals: ";
		if (at < n) return cl_fail(ctx, CL_E_MISMATCH, msg + "first at symbol " + std::to_string(at));
		if (size < 8) return cl_fail(ctx, CL_E_MISMATCH, msg + "a part has at least 8 bytes");
		// the part's triples (runs of TRIP_RUN, 64 places side by side) and bytes, for the count
		const uint64_t rows = ((uint64_t)n + TRIP_RUN - 1) / TRIP_RUN;
		std::vector<triple_t> t(rows * TRIP_RUN + 1); std::vector<uint8_t> b(size);
		uint64_t gb = 0, consumed = 0;
		HIP_TRY(ctx, hipMemcpy(&gb, d_gbase + (pl >> 6), 8, hipMemcpyDeviceToHost));
		if (rows) HIP_TRY(ctx, hipMemcpy2D(t.data(), TRIP_RUN * 8, trip + gb + (uint64_t)(pl & 63) * TRIP_RUN, 64ull * TRIP_RUN * 8, TRIP_RUN * 8, rows, hipMemcpyDeviceToHost));
		HIP_TRY(ctx, hipMemcpy(b.data(), d_out + dst_off[pl], size, hipMemcpyDeviceToHost));
		(void)rc_check_part_host(t.data(), n, b.data(), size, size, &consumed);
		return cl_fail(ctx, CL_E_MISMATCH, msg + "every symbol decodes, but the decoder consumes " + std::to_string(consumed) + " bytes and " + std::to_string(size) + " are stored");
	}
	return CL_OK;
}
#endif
