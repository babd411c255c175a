// digest.hpp — the content digest: what an archive must decode to, taken from the INPUT on the device at compress time
// (digest.hip), stored in the archive's `hipdigest` stream and recomputed on the host from what the decoders return (decode.hip,
// cli/reader.hpp).  Four digests — dna, qual, header, qual-values — of one shape, all arithmetic unsigned 64-bit and wrapping:
//     W(w_0 .. w_{m-1}) = sum_i mix(w_i + K (i + 1))            the words of one read
//     h                 = mix(W ^ mix(n + K kind))              n = symbols of the read
//     sum              += mix(h + K (g + 1))                    g = index of the read in the whole input
// Digests of disjoint sets of reads add field by field, in any order: chunks, lanes, domains and ranks combine by addition.
//
// qual-values (kind 4, opt-in: cl_ctx_set_digest_values) covers what the qual digest leaves out: the quality VALUES the decoders make
// of the symbols.  Per read one byte per base in read order, the value the decoder will write minus 33, eight to a word little-endian,
// the last word zero-padded; n = bases.  With q = input byte - 33 (outside 0..95: 0) and bin = map[q] (dg_qual_layout):
//     org      q                    2/4/5-fix   rev[bin] (-D)
//     2/4/5-avg, avg (one bin)      v_k = floor(k A / 256) - floor((k - 1) A / 256)          (dg_diffuse)
// with k = 1, 2, .. the rank of the base among the read's bases of its bin and A = the bin's two average bytes as one integer (dg_avg16:
// the code that forms them for k_digest_quals).  That IS the decoders' error diffusion `as += avg; v = (uint32)(as - qs); qs += v` with
// avg = A / 256 (quality_coder_impl.cpp:506-559,800-849): every partial sum is a multiple of 1/256 far below 2^53, so the double
// arithmetic is exact and qs after k steps is floor(k A / 256).  Integers only, and stated from the input.
//
// The step is written once, DG_HD, for the kernels and for the host loops.  Under a host compiler alone this header needs no HIP
// (tests/tools/digest_host_test.cpp; the public reader API is built that way).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/colord_hip.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DG_HD __host__ __device__
#else
#define DG_HD
#endif

enum { DG_DNA = 1, DG_QUAL = 2, DG_HEADER = 3, DG_QVAL = 4 };                 // `kind`
constexpr uint64_t DG_K = 0x9e3779b97f4a7c15ULL;

DG_HD inline uint64_t dg_mix(uint64_t x)
{
	x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
	x ^= x >> 27; x *= 0x94d049bb133111ebULL;
	x ^= x >> 31;
	return x;
}
DG_HD inline uint64_t dg_word(uint64_t w, uint64_t i) { return dg_mix(w + DG_K * (i + 1)); }                       // word i of a read: a term of W
DG_HD inline uint64_t dg_read(uint64_t W, uint64_t n, uint32_t kind) { return dg_mix(W ^ dg_mix(n + DG_K * kind)); } // h of a read
DG_HD inline uint64_t dg_term(uint64_t h, uint64_t g) { return dg_mix(h + DG_K * (g + 1)); }                       // the read's term of `sum`
// the packed bits under the invalid bases of a word: bit 31 - j of `inv` covers bits 63 - 2j and 62 - 2j
DG_HD inline uint64_t dg_spread(uint32_t inv)
{
	uint64_t x = inv;
	x = (x | (x << 16)) & 0x0000ffff0000ffffULL; x = (x | (x << 8)) & 0x00ff00ff00ff00ffULL;
	x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0fULL; x = (x | (x << 2)) & 0x3333333333333333ULL;
	x = (x | (x << 1)) & 0x5555555555555555ULL;
	return x | (x << 1);
}
// One 32-base block of the arena (cl_reads_packed / cl_reads_invalid) as the digest's two words: `rem` (1 .. 32 and more) bases of
// the read lie in it; everything behind them is cleared, and so are the packed bits under an N.
DG_HD inline void dg_block(uint64_t& packed, uint32_t& inv, uint64_t rem)
{
	if (rem < 32) { inv &= ~0u << (32 - (uint32_t)rem); packed &= ~0ULL << (64 - 2 * (uint32_t)rem); }
	packed &= ~dg_spread(inv);
}
// the k-th value (k = 1, 2, ..) the error diffusion of an average A / 256 gives (A <= 65535: k A stays below 2^64 for any k < 2^48)
DG_HD inline uint32_t dg_diffuse(uint32_t A, uint64_t k) { return (uint32_t)(((k * A) >> 8) - (((k - 1) * A) >> 8)); }
// the two average bytes of a bin as one integer, (a1 << 8) + a2: the average of cnt values that add up to sum, in 1/256 (quality_coder_impl.cpp:438-450)
DG_HD inline uint32_t dg_avg16(uint32_t sum, uint64_t cnt) { const double avg = cnt ? (double)sum / (double)cnt : 0.0; return (uint32_t)(avg * 256); }
// first_read + n must stay below 2^63
inline bool dg_range_ok(uint64_t first_read, uint64_t n) { return first_read < (1ULL << 63) && n <= (1ULL << 63) - first_read; }

// ---- host loops -------------------------------------------------------------------------------------------------------------
// One read at a time: bytes (ids; quality symbols) packed eight to a word little-endian, the last word zero-padded.
struct DigestFeed {
	uint64_t g = 0; cl_digest d{ 0, 0, 0 };
	uint64_t W = 0, word = 0, n = 0;
	void push(uint8_t s)
	{
		word |= (uint64_t)s << (8 * (n & 7));
		if ((++n & 7) == 0) { W += dg_word(word, n / 8 - 1); word = 0; }
	}
	void end_read(uint32_t kind)
	{
		if (n & 7) W += dg_word(word, n / 8);
		d.reads += 1; d.symbols += n; d.sum += dg_term(dg_read(W, n, kind), g++);
		W = word = n = 0;
	}
};
// n reads of base codes (low three bits: 0..3, 4 and above = N; the class flags the DNA decoder sets at levels 2 and 3 are ignored),
// read i at [h_off[i], h_off[i + 1]), the first of them read `first_read` of the input; added to *acc
inline bool dg_bases_host(const uint8_t* h_codes, const uint64_t* h_off, uint64_t n, uint64_t first_read, cl_digest* acc)
{
	if (!acc || (n && !h_off) || !dg_range_ok(first_read, n)) return false;
	for (uint64_t r = 0; r < n; ++r)
	{
		const uint8_t* p = h_codes + h_off[r]; const uint64_t len = h_off[r + 1] - h_off[r];
		uint64_t W = 0;
		for (uint64_t b = 0; 32 * b < len; ++b)
		{
			uint64_t P = 0; uint32_t N = 0;
			for (uint32_t j = 0; j < 32 && 32 * b + j < len; ++j)
			{
				const uint32_t c = p[32 * b + j] & 7;
				if (c >= 4) N |= 1u << (31 - j); else P |= (uint64_t)c << (62 - 2 * j);
			}
			W += dg_word(P, 2 * b) + dg_word(N, 2 * b + 1);
		}
		acc->reads += 1; acc->symbols += len; acc->sum += dg_term(dg_read(W, len, DG_DNA), first_read + r);
	}
	return true;
}
inline bool dg_bytes_host(uint32_t kind, const uint8_t* h_bytes, const uint64_t* h_off, uint64_t n, uint64_t first_read, cl_digest* acc)
{
	if (!acc || (n && !h_off) || kind < DG_DNA || kind > DG_HEADER || !dg_range_ok(first_read, n)) return false;
	DigestFeed f; f.g = first_read;
	for (uint64_t r = 0; r < n; ++r)
	{
		for (uint64_t i = h_off[r]; i < h_off[r + 1]; ++i) f.push(h_bytes[i]);
		f.end_read(kind);
	}
	acc->reads += f.d.reads; acc->symbols += f.d.symbols; acc->sum += f.d.sum;
	return true;
}

// ---- the quality symbols of a mode (QualityComprMode 0..8), as cl_qual_coder_create lays them out ----------------------------
// map[q - 33] = the per-base symbol; navg = the average bytes coded in front of a read's per-base symbols (avg: 2, and no per-base
// symbols); false: the thresholds do not fit the mode (cl_qual_coder_create refuses them the same way)
struct DigestQualLayout { uint32_t mode = 8, n_bins = 0, navg = 0, per_base = 0; uint8_t map[96]; };
// the bin of every Phred value 0..95 under n - 1 ascending thresholds <= 96 (adjust_quality_map_symbols, quality_coder.cpp:250-270): the one
// definition, for QualCfg::map_fwd of cl_qual_coder_create and for the digest
inline void qual_bin_map(uint8_t* map, const uint32_t* fwd, uint32_t n)
{
	for (uint32_t q = 0; q < fwd[0]; ++q) map[q] = 0;
	for (uint32_t b = 1; b < n; ++b) for (uint32_t q = fwd[b - 1]; q < (b + 1 < n ? fwd[b] : 96u); ++q) map[q] = (uint8_t)b;
}
inline bool dg_qual_layout(const cl_qual_params* prm, DigestQualLayout& L)
{
	if (!prm || prm->mode < 0 || prm->mode > 8) return false;
	L.mode = (uint32_t)prm->mode;
	for (int i = 0; i < 96; ++i) L.map[i] = prm->mode == 0 ? (uint8_t)i : 0;
	static const uint32_t bins_of[9] = { 0, 5, 4, 2, 5, 4, 2, 0, 0 };
	const uint32_t n = L.n_bins = bins_of[prm->mode];
	if (n)
	{
		if (prm->n_fwd != n - 1 || prm->fwd[n - 2] > 96) return false;
		for (uint32_t i = 0; i + 1 < n - 1; ++i) if (prm->fwd[i] > prm->fwd[i + 1]) return false;
		qual_bin_map(L.map, prm->fwd, n);
	}
	L.navg = prm->mode >= 1 && prm->mode <= 3 ? 2 * n : prm->mode == 7 ? 2u : 0u;
	L.per_base = prm->mode <= 6;
	return true;
}

// ---- the quality VALUES of a mode (qual-values, kind 4) --------------------------------------------------------------------------
// tab[q - 33]: org and *-fix the value itself (map and -D values composed); the diffusing modes (*-avg, avg) the bin (avg: one bin).
// false: dg_qual_layout refuses the parameters, mode none (no values are digested), more than 8 -D values (as cl_qual_decoder_create),
// a *-fix mode without a -D value for every bin, or a -D value that does not fit the byte the decoder writes (value + 33 <= 255).
struct DigestValueLayout { DigestQualLayout L; bool diffuse = false; uint32_t bins = 0; uint8_t tab[96]; };
inline bool dg_value_layout(const cl_qual_params* prm, DigestValueLayout& V)
{
	if (!dg_qual_layout(prm, V.L) || V.L.mode == 8 || prm->n_rev > 8) return false;
	const uint32_t m = V.L.mode;
	V.diffuse = (m >= 1 && m <= 3) || m == 7;
	V.bins = m == 7 ? 1u : V.L.n_bins;
	if (m >= 4 && m <= 6)
	{
		if (prm->n_rev < V.L.n_bins) return false;
		for (uint32_t b = 0; b < V.L.n_bins; ++b) if (prm->rev[b] > 222) return false;
	}
	for (int q = 0; q < 96; ++q) V.tab[q] = m == 0 ? (uint8_t)q : m == 7 ? 0 : V.diffuse ? V.L.map[q] : (uint8_t)prm->rev[V.L.map[q]];
	return true;
}
inline uint32_t dg_q_value(uint8_t byte) { const uint32_t q = (uint32_t)byte - 33u; return q > 95u ? 0u : q; }
// n reads of input quality bytes (Phred+33), read i at [h_off[i], h_off[i + 1]) -> the ASCII bytes the decoder will write for them, at
// the same offsets of h_values (null: not wanted), and their qual-values digest added to *acc (null: not wanted)
inline bool dg_qual_values_host(const cl_qual_params* prm, const uint8_t* h_quals, const uint64_t* h_off, uint64_t n, uint8_t* h_values, uint64_t first_read, cl_digest* acc)
{
	DigestValueLayout V;
	if (!dg_value_layout(prm, V) || (n && !h_off) || !dg_range_ok(first_read, n)) return false;
	DigestFeed f; f.g = first_read;
	for (uint64_t r = 0; r < n; ++r)
	{
		const uint8_t* q = h_quals + h_off[r]; const uint64_t len = h_off[r + 1] - h_off[r];
		uint32_t A[5] = { 0, 0, 0, 0, 0 }; uint64_t k[5] = { 0, 0, 0, 0, 0 };
		if (V.diffuse)
		{
			uint32_t sum[5] = { 0, 0, 0, 0, 0 }; uint64_t cnt[5] = { 0, 0, 0, 0, 0 };
			for (uint64_t i = 0; i < len; ++i) { const uint32_t v = dg_q_value(q[i]), b = V.tab[v]; sum[b] += v; cnt[b] += 1; }
			for (uint32_t b = 0; b < V.bins; ++b) A[b] = dg_avg16(sum[b], cnt[b]);
		}
		for (uint64_t i = 0; i < len; ++i)
		{
			const uint32_t t = V.tab[dg_q_value(q[i])], v = V.diffuse ? dg_diffuse(A[t], ++k[t]) : t;
			if (h_values) h_values[h_off[r] + i] = (uint8_t)(v + 33);
			f.push((uint8_t)v);
		}
		f.end_read(DG_QVAL);
	}
	if (acc) { acc->reads += f.d.reads; acc->symbols += f.d.symbols; acc->sum += f.d.sum; }
	return true;
}
// the qual-values digest of DECODED quality bytes (ASCII, value + 33, as a decoder hands them on): n reads at h_off, added to *acc
inline bool dg_qual_ascii_host(const uint8_t* h_ascii, const uint64_t* h_off, uint64_t n, uint64_t first_read, cl_digest* acc)
{
	if (!acc || (n && !h_off) || !dg_range_ok(first_read, n)) return false;
	DigestFeed f; f.g = first_read;
	for (uint64_t r = 0; r < n; ++r)
	{
		for (uint64_t i = h_off[r]; i < h_off[r + 1]; ++i) f.push((uint8_t)(h_ascii[i] - 33));
		f.end_read(DG_QVAL);
	}
	acc->reads += f.d.reads; acc->symbols += f.d.symbols; acc->sum += f.d.sum;
	return true;
}
