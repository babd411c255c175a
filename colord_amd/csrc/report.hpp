// report.hpp — the content report: what an archive holds — reads, bases, base composition, read lengths — and, for a
// coded quality stream, the exact joint distribution of INPUT quality against the quality VALUE the decoders will write (the quantity
// of the qual-values digest, digest.hpp).  Taken from the input on the device at compress time (report.hip); the host loops below
// state the same from host memory, for what a decoder returns and for the tests.  Every field of cl_report adds, except len_min /
// len_max (min / max) and has_qual (or): chunks, lanes, domains and ranks combine in any order.
//
// The arithmetic both sides share is written once, RP_HD.  Under a host compiler alone this header needs no HIP
// (tests/tools/report_host_test.cpp).
#pragma once
#include <string.h>
#include <algorithm>
#include <vector>
#include "digest.hpp"
#define RP_HD DG_HD

// bin of a read in len_hist / len_bases: the bit length of its length (0 -> 0, 1 -> 1, 2..3 -> 2, ..), 32 at the most
RP_HD inline uint32_t rp_len_bin(uint64_t len) { uint32_t b = 0; while (len && b < 32) { ++b; len >>= 1; } return b; }
// index of a quality (input: byte - 33; value: the byte the decoder writes - 33) in the histograms: outside 0..95 counts as 0 / stays at 95
RP_HD inline uint32_t rp_in(uint32_t byte) { const uint32_t q = byte - 33u; return q > 95u ? 0u : q; }
RP_HD inline uint32_t rp_out(uint32_t value) { return value > 95u ? 95u : value; }
// The counts of one 32-base block of the arena after dg_block (everything behind the read's end and the packed bits under an N
// cleared), `rem` (1 .. 32 and more) bases of the read lying in it: c[0..3] = A, C, G, T from popcounts on the two bit planes of
// `packed`, c[4] = N from the invalid mask
RP_HD inline uint32_t rp_popc64(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return (uint32_t)__popcll((unsigned long long)x);
#else
	return (uint32_t)__builtin_popcountll((unsigned long long)x);
#endif
}
RP_HD inline void rp_block_counts(uint64_t packed, uint32_t inv, uint64_t rem, uint32_t (&c)[5])
{
	const uint64_t LO = 0x5555555555555555ULL;
	const uint64_t hi = (packed >> 1) & LO, lo = packed & LO;
	const uint32_t in_read = rem < 32 ? (uint32_t)rem : 32u;
	c[4] = rp_popc64(inv);
	c[3] = rp_popc64(hi & lo); c[2] = rp_popc64(hi & ~lo); c[1] = rp_popc64(~hi & lo);
	c[0] = in_read - c[4] - c[3] - c[2] - c[1];
}

inline void rp_clear(cl_report* r) { memset(r, 0, sizeof(*r)); r->len_min = UINT64_MAX; }
inline void rp_add(cl_report* d, const cl_report* s)
{
	d->reads += s->reads; d->bases += s->bases;
	for (int i = 0; i < 5; ++i) d->base_count[i] += s->base_count[i];
	if (s->len_min < d->len_min) d->len_min = s->len_min;
	if (s->len_max > d->len_max) d->len_max = s->len_max;
	for (int i = 0; i < 33; ++i) { d->len_hist[i] += s->len_hist[i]; d->len_bases[i] += s->len_bases[i]; }
	d->has_qual |= s->has_qual;
	d->q_reads += s->q_reads; d->q_symbols += s->q_symbols;
	for (int i = 0; i < 96; ++i) d->mean_q_hist[i] += s->mean_q_hist[i];
	for (int i = 0; i < 96; ++i) for (int j = 0; j < 96; ++j) d->q_joint[i][j] += s->q_joint[i][j];
}
inline void rp_read_length(cl_report* a, uint64_t len)
{
	a->reads += 1; a->bases += len;
	if (len < a->len_min) a->len_min = len;
	if (len > a->len_max) a->len_max = len;
	const uint32_t b = rp_len_bin(len);
	a->len_hist[b] += 1; a->len_bases[b] += len;
}
// n reads of base codes (low three bits: 0..3, 4 and above = N), read i at [h_off[i], h_off[i + 1]): the content part, added to *acc.
// Through the same 32-base blocks and popcounts as the kernel.
inline bool rp_bases_host(const uint8_t* h_codes, const uint64_t* h_off, uint64_t n, cl_report* acc)
{
	if (!acc || (n && !h_off)) return false;
	for (uint64_t r = 0; r < n; ++r)
	{
		const uint8_t* p = h_codes + h_off[r]; const uint64_t len = h_off[r + 1] - h_off[r];
		for (uint64_t b = 0; 32 * b < len; ++b)
		{
			uint64_t P = 0; uint32_t N = 0;
			for (uint32_t j = 0; j < 32 && 32 * b + j < len; ++j)
			{
				const uint32_t c = p[32 * b + j] & 7;
				if (c >= 4) N |= 1u << (31 - j); else P |= (uint64_t)c << (62 - 2 * j);
			}
			uint32_t c[5];
			rp_block_counts(P, N, len - 32 * b, c);
			for (int t = 0; t < 5; ++t) acc->base_count[t] += c[t];
		}
		rp_read_length(acc, len);
	}
	return true;
}
// the value layout of a mode for the report: dg_value_layout, and every -D value of a *-fix mode must be a quality 0..95
inline bool rp_value_layout(const cl_qual_params* prm, DigestValueLayout& V)
{
	if (!dg_value_layout(prm, V)) return false;
	if (V.L.mode >= 4 && V.L.mode <= 6) for (uint32_t b = 0; b < V.L.n_bins; ++b) if (prm->rev[b] > 95) return false;
	return true;
}
// n reads of INPUT quality bytes (Phred+33): the quality part — q_joint[in][out] with `out` the value a decoder of `prm` will write,
// mean_q_hist from the input — added to *acc.  Mode none: true, nothing added.
inline bool rp_quals_host(const cl_qual_params* prm, const uint8_t* h_quals, const uint64_t* h_off, uint64_t n, cl_report* acc)
{
	if (!prm || !acc || (n && !h_off)) return false;
	if (prm->mode == 8) return true;
	DigestValueLayout V;
	if (!rp_value_layout(prm, V)) return false;
	acc->has_qual = 1;
	for (uint64_t r = 0; r < n; ++r)
	{
		const uint8_t* q = h_quals + h_off[r]; const uint64_t len = h_off[r + 1] - h_off[r];
		uint32_t A[5] = { 0, 0, 0, 0, 0 }; uint64_t k[5] = { 0, 0, 0, 0, 0 };
		if (V.diffuse)
		{
			uint32_t sum[5] = { 0, 0, 0, 0, 0 }; uint64_t cnt[5] = { 0, 0, 0, 0, 0 };
			for (uint64_t i = 0; i < len; ++i) { const uint32_t v = rp_in(q[i]), b = V.tab[v]; sum[b] += v; cnt[b] += 1; }
			for (uint32_t b = 0; b < V.bins; ++b) A[b] = dg_avg16(sum[b], cnt[b]);
		}
		uint64_t total = 0;
		for (uint64_t i = 0; i < len; ++i)
		{
			const uint32_t in = rp_in(q[i]), t = V.tab[in], v = V.diffuse ? dg_diffuse(A[t], ++k[t]) : t;
			acc->q_joint[in][rp_out(v)] += 1; total += in;
		}
		acc->q_reads += 1; acc->q_symbols += len;
		if (len) acc->mean_q_hist[rp_out((uint32_t)(total / len))] += 1;
	}
	return true;
}
// n reads of DECODED quality bytes (ASCII, as a decoder hands them on): q_reads, q_symbols and the OUT marginal alone — every base is
// counted in row 0, q_joint[0][out], so the column sums are the marginal; the IN side of such a report says nothing
inline bool rp_values_host(const uint8_t* h_ascii, const uint64_t* h_off, uint64_t n, cl_report* acc)
{
	if (!acc || (n && !h_off)) return false;
	acc->has_qual = 1;
	for (uint64_t r = 0; r < n; ++r)
	{
		for (uint64_t i = h_off[r]; i < h_off[r + 1]; ++i) acc->q_joint[0][rp_out((uint32_t)(uint8_t)(h_ascii[i] - 33))] += 1;
		acc->q_reads += 1; acc->q_symbols += h_off[r + 1] - h_off[r];
	}
	return true;
}
// N50 / N90 are not additive: from all read lengths (sorted here, descending), the length at which the running sum of bases first
// reaches 50 % / 90 % of all bases (0 without bases).  pct 1..100.
inline uint64_t rp_nxx(std::vector<uint64_t> lens, uint32_t pct)
{
	std::sort(lens.begin(), lens.end(), [](uint64_t a, uint64_t b) { return a > b; });
	unsigned __int128 total = 0; for (uint64_t l : lens) total += l;
	unsigned __int128 run = 0;
	for (uint64_t l : lens) { run += l; if (l && run * 100 >= total * pct) return l; }
	return 0;
}
