// qual_walk.hpp — the walk over one read's quality bytes that gives every byte the VALUE the decoders will write for it (digest.hpp,
// qual-values), written once for its two users: k_qual_values (digest.hip: digest and / or store the values) and k_report_quals
// (report.hip: count input quality against value).  Device code only.
#pragma once
#include "common.hpp"
#include "digest.hpp"

__device__ inline uint64_t wave_sum64(uint64_t v)
{
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
	return v;
}
__device__ inline uint64_t wave_incl_scan64(uint64_t v, uint32_t lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) { const uint64_t t = (uint64_t)__shfl_up((unsigned long long)v, d, 64); if ((int)lane >= d) v += t; }
	return v;
}
// eight quality bytes from index i of a read (i + 8 <= len): one unaligned 8-byte load inside the read
__device__ inline uint64_t load_q8(const uint8_t* __restrict__ q, uint64_t i) { uint64_t v; __builtin_memcpy(&v, q + i, 8); return v; }
__device__ inline uint32_t q_value(uint32_t byte) { const uint32_t q = byte - 33u; return q > 95u ? 0u : q; }     // (outside Phred+33 0..95: as k_qual_symbols, which makes cl_qual_encode refuse the input)

// Pass one of the averaging modes, for k_digest_quals and the value walk: the wave's per-bin integer sums and counts of the read q[0 .. len),
// then a[t] = the two average bytes of bin t as one integer (dg_avg16; 0 for an empty bin and for t >= bins).  one_bin (avg): every base in bin 0.
__device__ inline void bin_averages(const uint8_t* s_map, bool one_bin, uint32_t bins, const uint8_t* __restrict__ q, uint64_t len, uint32_t lane, uint32_t (&a)[5])
{
	uint32_t sum[5] = { 0, 0, 0, 0, 0 }, cnt[5] = { 0, 0, 0, 0, 0 };
	auto count = [&](uint32_t byte) {
		const uint32_t v = q_value(byte), b = one_bin ? 0u : s_map[v];
#pragma unroll
		for (uint32_t t = 0; t < 5; ++t) if (b == t) { sum[t] += v; cnt[t] += 1; }
	};
	for (uint64_t i = 8ull * lane; i < len; i += 512)
	{
		if (i + 8 <= len) { const uint64_t v = load_q8(q, i);
#pragma unroll
			for (uint32_t k = 0; k < 8; ++k) count((uint32_t)(v >> (8 * k)) & 0xffu); }
		else for (uint64_t j = i; j < len; ++j) count(q[j]);
	}
#pragma unroll
	for (uint32_t t = 0; t < 5; ++t) { sum[t] = wave_sum(sum[t]); cnt[t] = wave_sum(cnt[t]); }
#pragma unroll
	for (uint32_t t = 0; t < 5; ++t) a[t] = t < bins ? dg_avg16(sum[t], one_bin ? len : (uint64_t)cnt[t]) : 0u;
}

// tab8: the 96-entry table of dg_value_layout — the value itself (org, *-fix) or the bin (diffuse: *-avg, avg)
struct QualValueArg { uint32_t diffuse, bins; uint64_t tab8[12]; };

// One wave walks one read, q[0 .. len); every lane of the wave calls this (the diffusing modes scan over the wave).  Lane l of step s
// holds group i = 64 s + l: the bytes 8 i .. 8 i + 7 of the read (one 8-byte load; the last, partial group byte by byte).  For every
// group that holds bytes, emit(in, values, i, nb): `in` the nb input bytes as they stand (ASCII, low byte first, the rest zero), `values`
// the value of each (the byte the decoder writes minus 33) at the same place.  org / *-fix: a table look-up per byte.  Diffusing modes:
// pass one gives A per bin (bin_averages); then per step every lane counts its bytes per bin into one word of five 10-bit fields (a step
// holds <= 512 bytes), ONE 64-bit wave scan gives it the rank of its first byte in every bin within the step, the bins' totals of the
// steps before are five wave-uniform 64-bit counters, and the lane walks its bytes in registers: k = carried + before + 1, 2, ..;
// v = dg_diffuse(A, k).  Every loop bound is known before the loop; nothing outside q[0 .. len) is loaded.
template<typename Emit>
__device__ inline void qual_value_walk(const QualValueArg& cfg, const uint8_t* s_tab, const uint8_t* __restrict__ q, uint64_t len, uint32_t lane, Emit&& emit)
{
	const uint64_t words = (len + 7) / 8, steps = (words + 63) / 64;
	if (!cfg.diffuse)
	{
		for (uint64_t i = lane; i < words; i += 64)
		{
			const uint64_t j0 = 8 * i;
			uint64_t v = 0, w = 0; uint32_t nb = 8;
			if (j0 + 8 <= len)
			{
				v = load_q8(q, j0);
#pragma unroll
				for (uint32_t k = 0; k < 8; ++k) w |= (uint64_t)s_tab[q_value((uint32_t)(v >> (8 * k)) & 0xffu)] << (8 * k);
			}
			else
			{
				nb = (uint32_t)(len - j0);
				for (uint32_t k = 0; k < nb; ++k) { const uint32_t b = q[j0 + k]; v |= (uint64_t)b << (8 * k); w |= (uint64_t)s_tab[q_value(b)] << (8 * k); }
			}
			emit(v, w, i, nb);
		}
	}
	else
	{
		uint32_t A[5];
		bin_averages(s_tab, cfg.bins == 1, cfg.bins, q, len, lane, A);
		uint64_t carried[5] = { 0, 0, 0, 0, 0 };                               // per bin: the read's bases of the steps before (wave-uniform)
		for (uint64_t s = 0; s < steps; ++s)                                    // (wave-uniform: every lane takes part in the scan)
		{
			const uint64_t i = 64 * s + lane, j0 = 8 * i;
			uint64_t v = 0; uint32_t nb = 0;
			if (j0 + 8 <= len) { v = load_q8(q, j0); nb = 8; }
			else if (j0 < len) { nb = (uint32_t)(len - j0); for (uint32_t k = 0; k < nb; ++k) v |= (uint64_t)q[j0 + k] << (8 * k); }
			uint32_t bins = 0; uint64_t mine = 0;                               // the bins of the lane's bytes, 3 bits each; its count per bin, 10 bits each
#pragma unroll
			for (uint32_t k = 0; k < 8; ++k) if (k < nb)
			{
				const uint32_t b = s_tab[q_value((uint32_t)(v >> (8 * k)) & 0xffu)];
				bins |= b << (3 * k); mine += 1ULL << (10 * b);
			}
			const uint64_t incl = wave_incl_scan64(mine, lane), before = incl - mine;
			const uint64_t total = (uint64_t)__shfl((unsigned long long)incl, 63, 64);
			uint64_t k_of[5];
#pragma unroll
			for (uint32_t t = 0; t < 5; ++t) k_of[t] = carried[t] + ((before >> (10 * t)) & 1023u);
			uint64_t w = 0;
#pragma unroll
			for (uint32_t k = 0; k < 8; ++k) if (k < nb)
			{
				const uint32_t b = (bins >> (3 * k)) & 7u;
				uint64_t kk = 0; uint32_t a = 0;
#pragma unroll
				for (uint32_t t = 0; t < 5; ++t) if (b == t) { kk = ++k_of[t]; a = A[t]; }
				w |= (uint64_t)dg_diffuse(a, kk) << (8 * k);
			}
			if (nb) emit(v, w, i, nb);
#pragma unroll
			for (uint32_t t = 0; t < 5; ++t) carried[t] += (total >> (10 * t)) & 1023u;
		}
	}
}
